#!/usr/bin/env python3
"""Generator of the hand-scheduled bf16 GEMM kernels for gfx950 (gemm_asm_kernel_*, longlive_amd/csrc/gemm_asm.hip):
Y[M, N] = epilogue(X[M, K] . W[N, K]^T + bias), the block linears of wan/modules/causal_model.py:406-408 (ffn.0 + GELU),
:456,467 (ffn.2 / o + gate-residual), model.py:172,192-193 (cross o / q).

Same construction as the attention kernel (gen/attn_asm_gen.py: one asm statement of generated text, one wave per SIMD owning
the 512-register file, fillers placed between MFMAs, LDS waits by a dependency pass, hazard linter, executed by
tools/gfx950_emu.py in the CPU suite before any GPU run):

  * workgroup = 4 waves = a 256 (M) x WN (N) output tile; wave w owns rows 64 w .. 64 w + 63 and ALL WN columns:
    accumulators acc[mb][nb] (mb < 2, nb < WN / 32) = 2 WN / 32 tiles of 32 x 32 in AGPRs (224 registers at WN = 224).
    Operands are swapped as in gemm.hip (A := W rows = output columns, B := X rows): a lane then owns ONE output row
    (m = lane & 31) and, per 32-column block, columns 8 g + 4 h + (0..3) -- 8-byte runs that one v_permlane32_swap per pair
    turns into 16-byte stores (T21).
  * the loop runs in half-steps of 32 K (two MFMA k-steps, 2 NB x 2 MFMAs); W fragments of half-step h + 1 are read from LDS into
    the other half of a double-buffered fragment file while the MFMAs of half-step h run; every W fragment feeds two MFMAs, every
    X fragment WN / 32.
  * ONLY W goes through LDS (it is what the four waves share): a ring of 5 slots of one 64-deep K-step each (WN rows x 128 B =
    whole cache lines, XOR-swizzled on the SOURCE address: chunk ^ ((row >> 1) & 7)), staged by buffer_load ... lds four K-steps
    ahead.  A wave's 64 X rows are its own: its X fragments come STRAIGHT from global memory into a 5-deep register ring
    (4 buffer_load_dwordx4 per half-step, four half-steps ahead).  Descriptors bound the ROWS (rows past M / N read as zeros), the
    K offset travels in soffset.  (The first form staged X through LDS as well, in a 4-slot ring of 32 KiB: correct, but latency-
    bound at 15 B/clk of staging per CU -- no faster than the HIP kernels.)  vmcnt is one in-order queue: the wait at the end of
    a half-step is counted so that the next half-step's X fragments -- and with them every W piece older than ~3 half-steps --
    have landed; one barrier per K-step.
  * MFMA shape (Cfg.mfma, bf16 texts only): 32 = v_mfma_f32_32x32x16_bf16 as described above; 16 = v_mfma_f32_16x16x32_bf16 at the SAME
    output tile per wave, accumulator count, LDS image, staging, waits and tile walk: one MFMA per (16-column W block, 16-row X block)
    and half-step, fragments read as row l & 15 / 16 bytes of K at 16 (l >> 4) of the 64-byte half line (as many ds_read_b128 and
    bytes; conflict-free under the same XOR swizzle, tests/test_gemm_asm_mfma16_emu.py), twice as many 16-cycle gaps for the same
    fillers; v_permlane16_swap between the two 16-row blocks of a 32-row block gives the epilogue the 16-byte runs of the 32-shape.
    Text for mfma = 32 is byte-identical to the generator before the parameter existed.
  * epilogues in the same text, rounding points as gemm_common.h (v = bf16(acc + bias); GELU x.sigma(2u) with v_exp / v_rcp;
    x + bf16(v . gate[frame]); x + v), packed-f32 VALU where it halves the instruction count (no MFMA runs beside it).
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_asm_gen as _A                                                                     # noqa: E402
from attn_asm_gen import Gen, finalize, lint, sreg, vreg, areg, to_inc, f32bits, spread   # noqa: E402

EPI_BIAS, EPI_GELU, EPI_GATE_RES, EPI_RES = 0, 1, 2, 3
EPI_PARTIAL = 4                                                   # no epilogue: the raw fp32 accumulators (one K-range of a split-K call), Y = float [rows, ldo / 4]
EPI_BIAS_SSQ = 5                                                  # EPI_BIAS + per-row sum of squares of the tile's bf16 outputs -> ssq[row] (fp32): the statistics of
                                                                  # the RMSNorm that follows the projection (WanRMSNorm, wan/modules/model.py:78-86 after :172), summed
                                                                  # over the n-tiles and applied by the consumer (flash_attn_asm_qn_kernel's Q prologue)

# ---- inputs (pinned by the HIP wrapper) ----------------------------------------------------------------------------
S_X, S_W, S_Y, S_BIAS, S_RES, S_GATE = 8, 10, 12, 14, 16, 18      # 64-bit bases (bytes): X row m0; W row n0; Y / RES at (m0, n0); bias + n0;
                                                                  # gate table e + gate_idx * N + n0 (row stride S_GSTRIDE per frame)
S_LDX, S_LDW, S_LDO = 20, 21, 22                                  # row strides in bytes
S_ROWS, S_COLS, S_NK = 23, 24, 25                                 # valid rows (M - m0), valid columns (N - n0, >= WN on this path), K / 64
S_FLEN, S_GSTRIDE, S_M0 = 26, 27, 28                              # gate: frame_len (rows per frame), bytes between frames' gate rows, m0
S_ROWLO = 29                                                      # first row of the tile that is stored (0 except in V tiles of the fused QKV projection)
S_SX, S_SW = 64, 66                                               # W8A8 kernels: 64-bit bases of the activation scales (sx + m0) and weight scales (sw + n0), fp32
S_SSQ = 64                                                        # EPI_BIAS_SSQ (bf16 only): 64-bit base of this tile's row sums, fp32 [rows] (ssq + n_tile * M + m0)
# working scalars
S_XRS, S_WRS = 32, 36                                             # descriptors
S_WAVE, S_I, S_T0, S_T1, S_T2 = 40, 41, 44, 45, 46
S_WM0, S_XK, S_WK, S_XKMAX, S_WKMAX = 47, 48, 49, 43, 62
S_MSK = 50                                                        # 64-bit lane masks s[50:51], s[52:53]
V_TID = 0

NSLOT, XU = 3, 2                                                  # W ring slots (shared, one 64-deep K-step each); X units per wave (private)
S_XM0 = 30                                                        # LDS base of this wave's X units

# ---- PERSISTENT form (bf16; generate(..., persistent=True)): a workgroup walks tiles S_TILE, S_TILE + S_GRID, ... of the launch and
# issues the NEXT tile's first staging pieces (W(0..2), X(0..1)) before the current tile's epilogue, so a launch of several rounds
# (FFN1: 760 tiles, QKV: 456 on 256 CUs) pays one pipeline fill, and the epilogue's VALU time runs over the next tile's staging.
# Inputs are the MATRIX bases; the per-tile scalars above (S_X ... S_ROWLO, S_LDO) are computed here from the tile index with
# gemm_common.h's mapping (xcd_remap + tile_of), including the V-cache redirect of the fused QKV projection.
S_XB, S_WB, S_YB, S_BIASB, S_RESB, S_GATEB = 84, 86, 88, 90, 92, 94      # 64-bit bases: X, W, Y, bias, res, gate table (+ gate_idx * N)
S_LDO0, S_MM, S_NN = 68, 69, 70                                   # Y / RES row stride in bytes; M; N
S_TILE, S_GRID, S_NTILES, S_NTM, S_NTN, S_GM = 71, 72, 73, 74, 75, 76     # this workgroup's tile, tile stride, tiles, m-tiles, n-tiles, m-tiles per group (>= 1)
S_VHI, S_VOUT, S_VCOL0, S_VC2, S_VSHIFT, S_VLO = 77, 78, 80, 81, 82, 83  # V redirect: v_hi; s[78:79] cache_v (0 = none); first V column; cache row stride in
                                                                  # BYTES; cache row of token 0 (signed); v_lo
S_XN, S_WN, S_PF, S_ROWSN = 64, 66, 31, 42                        # next tile: X / W bases; 1 = its first pieces are staged; its valid rows
S_MT, S_NT = 54, 55                                               # (m-tile, n-tile) of the tile being mapped; s[54:61] + S_T0..2 are the mapping's scratch


def KN(k):
    """timing-only experiment switches (ASM_G_<k>=1; results are invalid with any of them set): refused without --diag
    (attn_asm_gen.knob_env)"""
    return _A.knob_env("ASM_G_", k, 0)


class Cfg:
    def __init__(self, WN, epi, i8=False, mfma=32):
        assert WN % 32 == 0 and 64 <= WN <= 256
        assert not (i8 and epi in (EPI_PARTIAL, EPI_BIAS_SSQ))
        assert mfma in (32, 16) and not (mfma == 16 and (i8 or epi == EPI_PARTIAL))
        self.WN, self.NB, self.MB, self.epi, self.i8 = WN, WN // 32, 2, epi, i8
        self.mfma = mfma                                          # bf16 MFMA shape: 32 = v_mfma_f32_32x32x16_bf16, 16 = v_mfma_f32_16x16x32_bf16 (same output tile
        self.m16 = mfma == 16                                     # per wave, same registers; see mfmas() for the layout)
        self.sc = 2 if self.m16 else 1                            # MFMAs per half-step relative to the 32-shape: filler positions scale with it
        self.bl = 2 if self.m16 else 4                            # bias loads (8 bytes per lane each) per 32-column block
        self.nacc = self.MB * self.NB * 16
        self.slotb = WN * 128                                      # bytes of one W slot: WN rows x 128 B (a 64-deep K-step)
        self.npw = WN // 32                                        # 1-KiB LDS-DMA pieces of W per wave and K-step (WN / 8 pieces of 8 rows)
        self.xbase = NSLOT * self.slotb                            # X units follow the W ring: wave w, unit u at xbase + (XU w + u) * xunit
        self.xunit = 64 * 128                                      # a wave's 64 rows x 128 B
        self.lds_bytes = self.xbase + 4 * XU * self.xunit
        assert self.lds_bytes <= 160 * 1024
        # VGPR map
        self.FW = 0                                               # FW[p][nb][ks]: 4 registers each, p = half-step parity
        self.FX = 2 * self.NB * 2 * 4                             # FX[b][mb][ks4]: b = K-step parity, ks4 = 0..3 (a whole K-step)
        nxt = max(self.FX + 2 * self.MB * 4 * 4, 144)             # (the epilogue's 72 temporaries + setup scratch live below)
        self.V_WOFF = nxt                                         # [base64k][hs][ks] -> 12 registers
        self.V_XROFF = nxt + 12                                   # [ks4] X fragment read addresses
        self.V_DW = nxt + 16                                      # W DMA source offsets, npw <= 8 pieces
        self.V_DX = nxt + 24                                      # X DMA source offsets, 8 pieces
        self.V_LANE, self.V_R, self.V_H, self.V_ROW = nxt + 32, nxt + 33, nxt + 34, nxt + 35      # V_ROW[mb] -> +35, +36
        self.V_T = 0                                              # epilogue temporaries re-use the fragment file
        assert nxt + 37 <= 256, nxt
        # registers above the loop's own: epilogue addresses (computed before the loop) and the epilogue's EARLY reads -- bias
        # vectors of the first `early_nb` column blocks and the first block's gate / residual pieces are fetched before the
        # first staging piece, so the epilogue starts without an exposed memory latency
        self.V_EA = nxt + 37                                      # +0,+1 row byte offsets in Y / RES; +2 bias column offset; +3,+4 gate row offsets
        top = self.V_EA + (7 if self.m16 else 5)                  # (16-shape: +3..+6, one gate row offset per 16-row block)
        if i8:                                                    # W8A8: +5 column byte offset into the weight scales (16 h); V_SX[mb] = (sx[row], sx[row]) pairs
            self.V_SX = top + 2                                   # (register pairs start on even registers)
            top += 6
        assert top % 2 == 0, top
        self.nl = {EPI_GATE_RES: 6, EPI_RES: 2}.get(epi, 0)       # global reads per epilogue block
        self.V_E0 = top                                           # the first block's gate / residual pieces (16 registers) when nl
        top += 16 if self.nl else 0
        self.V_SS = top                                           # EPI_BIAS_SSQ: running sums of squares SS[mb] = 2 registers each (even / odd column of a pair)
        top += (8 if self.m16 else 4) if epi == EPI_BIAS_SSQ else 0      # (16-shape: SS[mb16], a lane's accumulators span two rows per 32-row block)
        self.V_EB = top                                           # early bias [nb][g4], 2 registers each
        self.early_nb = 0 if epi == EPI_PARTIAL else max(0, min(self.NB, (256 - top) // 8))

    def acc(self, mb, nb):
        return (mb * self.NB + nb) * 16

    def fw(self, p, nb, ks):
        return self.FW + ((p * self.NB + nb) * 2 + ks) * 4

    def fx(self, b, mb, ks4):
        return self.FX + ((b * self.MB + mb) * 4 + ks4) * 4

    # 16-shape: the same files cut into 16-row blocks -- acc16[mb16][nb16] (4 registers), FW16[p][nb16], FX16[b][mb16][hs]
    def acc16(self, mb16, nb16):
        return (mb16 * 2 * self.NB + nb16) * 4

    def fw16(self, p, nb16):
        return self.FW + (p * 2 * self.NB + nb16) * 4

    def fx16(self, b, mb16, hs):
        return self.FX + ((b * 4 + mb16) * 2 + hs) * 4


def mfmas(c: Cfg, h):
    p, b, hf = h & 1, (h >> 1) & 1, h & 1
    out = []
    if c.m16:
        # one MFMA per (16-column W block, 16-row X block) covers the half-step's 32 K: lane l feeds row l & 15 and the 16 bytes of K
        # at 16 (l >> 4) of the 64-byte half line, and ends up with row m = 16 mb16 + (l & 15), columns 16 nb16 + 4 (l >> 4) + (0..3).
        # nb16 outer: a W fragment feeds four consecutive MFMAs, no two consecutive MFMAs share an accumulator.
        for nb16 in range(2 * c.NB):
            for mb16 in range(4):
                a = areg(c.acc16(mb16, nb16), 4)
                out.append(f"v_mfma_f32_16x16x32_bf16 {a}, {vreg(c.fw16(p, nb16), 4)}, {vreg(c.fx16(b, mb16, hf), 4)}, {a}")
        return out
    for ks in range(2):
        for nb in range(c.NB):
            for mb in range(c.MB):
                a = areg(c.acc(mb, nb), 16)
                op = "v_mfma_i32_32x32x32_i8" if c.i8 else "v_mfma_f32_32x32x16_bf16"      # same operand registers: 16 B of K per lane and MFMA
                out.append(f"{op} {a}, {vreg(c.fw(p, nb, ks), 4)}, {vreg(c.fx(b, mb, 2 * hf + ks), 4)}, {a}")
    return out


def w_frag_reads(c: Cfg, h):
    """W fragments of half-step h (K-step h >> 1, half h & 1) from its ring slot into FW[h & 1]"""
    slot, hs = (h >> 1) % NSLOT, h & 1
    out = []
    if c.m16:                                                     # as many reads and bytes as below: one per 16-row block (2 KiB apart) and half-step
        for nb16 in range(2 * c.NB):
            off = slot * c.slotb + nb16 * 2048
            b64, imm = off >> 16, off & 0xFFFF
            out.append(f"ds_read_b128 {vreg(c.fw16(h & 1, nb16), 4)}, {vreg(c.V_WOFF + 4 * b64 + 2 * hs)} offset:{imm}")
        return out
    for ks in range(2):
        for nb in range(c.NB):
            off = slot * c.slotb + nb * 4096
            b64, imm = off >> 16, off & 0xFFFF
            out.append(f"ds_read_b128 {vreg(c.fw(h & 1, nb, ks), 4)}, {vreg(c.V_WOFF + 4 * b64 + 2 * hs + ks)} offset:{imm}")
    return out


def x_frag_reads(c: Cfg, s):
    """the wave's X fragments of K-step s (both half-steps) from its own unit s % XU into FX[s & 1]"""
    out = []
    if c.m16:
        for hs in range(2):
            for mb16 in range(4):
                out.append(f"ds_read_b128 {vreg(c.fx16(s & 1, mb16, hs), 4)}, {vreg(c.V_XROFF + 2 * hs)} offset:{(s % XU) * c.xunit + mb16 * 2048}")
        return out
    for ks4 in range(4):
        for mb in range(c.MB):
            out.append(f"ds_read_b128 {vreg(c.fx(s & 1, mb, ks4), 4)}, {vreg(c.V_XROFF + ks4)} offset:{(s % XU) * c.xunit + mb * 4096}")
    return out


def x_dma(c: Cfg, s):
    """the wave's 64 X rows of K-step s (8 pieces of 8 rows x 128 B: whole cache lines) into its own unit s % XU"""
    out = []
    for i in range(8):
        out.append(f"s_add_u32 m0, {sreg(S_XM0)}, {(s % XU) * c.xunit + 1024 * i}")
        out.append(f"buffer_load_dwordx4 {vreg(c.V_DX + i)}, {sreg(S_XRS, 4)}, {sreg(S_XK)} offen lds")
    out.append(f"s_add_u32 {sreg(S_XK)}, {sreg(S_XK)}, 128")
    out.append(f"s_min_u32 {sreg(S_XK)}, {sreg(S_XK)}, {sreg(S_XKMAX)}")           # past the end: re-load the last K-step (never read)
    return out


def w_dma(c: Cfg, s):
    """this wave's pieces of W K-step s into ring slot s % NSLOT"""
    out = []
    for i in range(c.npw):
        out.append(f"s_add_u32 m0, {sreg(S_WM0)}, {(s % NSLOT) * c.slotb + 1024 * i}")
        out.append(f"buffer_load_dwordx4 {vreg(c.V_DW + i)}, {sreg(S_WRS, 4)}, {sreg(S_WK)} offen lds")
    out.append(f"s_add_u32 {sreg(S_WK)}, {sreg(S_WK)}, 128")
    out.append(f"s_min_u32 {sreg(S_WK)}, {sreg(S_WK)}, {sreg(S_WKMAX)}")
    return out


def drop_loads(ops):
    return [o for o in ops if not o.startswith("buffer_load")]


def udiv(g: Gen, q, num, den, T):
    """SGPR q = num / den (unsigned, num < 2^24) for wave-uniform SGPR operands: float estimate on the VALU, one correction each way"""
    I = g.I
    I(f"v_cvt_f32_u32 {vreg(T)}, {sreg(num)}")
    I(f"v_cvt_f32_u32 {vreg(T + 1)}, {sreg(den)}")
    I(f"v_rcp_f32 {vreg(T + 1)}, {vreg(T + 1)}")
    I("s_nop 0")
    I(f"v_mul_f32 {vreg(T)}, {vreg(T)}, {vreg(T + 1)}")
    I(f"v_cvt_u32_f32 {vreg(T)}, {vreg(T)}")
    I("s_nop 0")
    I(f"v_readfirstlane_b32 {sreg(q)}, {vreg(T)}")
    I("s_nop 0")
    I(f"s_mul_i32 {sreg(S_T2)}, {sreg(q)}, {sreg(den)}")
    I(f"s_cmp_gt_u32 {sreg(S_T2)}, {sreg(num)}")                   # estimate one too big
    I(f"s_cselect_b32 {sreg(S_T2)}, 1, 0")
    I(f"s_sub_u32 {sreg(q)}, {sreg(q)}, {sreg(S_T2)}")
    I(f"s_mul_i32 {sreg(S_T2)}, {sreg(q)}, {sreg(den)}")
    I(f"s_sub_u32 {sreg(S_T2)}, {sreg(num)}, {sreg(S_T2)}")        # remainder so far
    I(f"s_cmp_ge_u32 {sreg(S_T2)}, {sreg(den)}")                   # estimate one too small
    I(f"s_cselect_b32 {sreg(S_T2)}, 1, 0")
    I(f"s_add_u32 {sreg(q)}, {sreg(q)}, {sreg(S_T2)}")


def gen_tile_map(g: Gen, tile, T):
    """S_MT, S_NT <- tile_of(xcd_remap(tile, S_NTILES), S_NTM, S_NTN, S_GM) (gemm_common.h).  Clobbers s[54:61], S_T0..2, v[T:T+1]."""
    I = g.I
    q, r, x, hi, q1, a, b, c_ = 54, 55, 56, 57, 58, 59, 60, 61
    I(f"s_lshr_b32 {sreg(q)}, {sreg(S_NTILES)}, 3")
    I(f"s_and_b32 {sreg(r)}, {sreg(S_NTILES)}, 7")
    I(f"s_and_b32 {sreg(x)}, {sreg(tile)}, 7")
    I(f"s_lshr_b32 {sreg(hi)}, {sreg(tile)}, 3")
    I(f"s_add_u32 {sreg(q1)}, {sreg(q)}, 1")
    I(f"s_mul_i32 {sreg(a)}, {sreg(x)}, {sreg(q1)}")                # xcd < r:  xcd * (q + 1)
    I(f"s_mul_i32 {sreg(b)}, {sreg(r)}, {sreg(q1)}")                # else:     r * (q + 1) + (xcd - r) * q
    I(f"s_sub_u32 {sreg(c_)}, {sreg(x)}, {sreg(r)}")
    I(f"s_mul_i32 {sreg(c_)}, {sreg(c_)}, {sreg(q)}")
    I(f"s_add_u32 {sreg(b)}, {sreg(b)}, {sreg(c_)}")
    I(f"s_cmp_lt_u32 {sreg(x)}, {sreg(r)}")
    I(f"s_cselect_b32 {sreg(a)}, {sreg(a)}, {sreg(b)}")
    I(f"s_add_u32 {sreg(S_T0)}, {sreg(a)}, {sreg(hi)}")             # lid
    # tile_of: per = gm * ntn; g = lid / per; first = g * gm; gs = min(ntm - first, gm); w = lid - g * per; nt = w / gs; mt = first + w % gs
    I(f"s_mul_i32 {sreg(S_T1)}, {sreg(S_GM)}, {sreg(S_NTN)}")       # per
    udiv(g, 56, S_T0, S_T1, T)                                      # s56 = g
    I(f"s_mul_i32 {sreg(57)}, {sreg(56)}, {sreg(S_T1)}")
    I(f"s_sub_u32 {sreg(S_T0)}, {sreg(S_T0)}, {sreg(57)}")          # w
    I(f"s_mul_i32 {sreg(58)}, {sreg(56)}, {sreg(S_GM)}")            # first
    I(f"s_sub_u32 {sreg(S_T1)}, {sreg(S_NTM)}, {sreg(58)}")
    I(f"s_min_u32 {sreg(S_T1)}, {sreg(S_T1)}, {sreg(S_GM)}")        # gs
    udiv(g, S_NT, S_T0, S_T1, T)                                    # nt = w / gs
    I(f"s_mul_i32 {sreg(57)}, {sreg(S_NT)}, {sreg(S_T1)}")
    I(f"s_sub_u32 {sreg(57)}, {sreg(S_T0)}, {sreg(57)}")            # w % gs
    I(f"s_add_u32 {sreg(S_MT)}, {sreg(58)}, {sreg(57)}")


def add64(g: Gen, dst, base, lo, hi=None):
    """s[dst:dst+1] = s[base:base+1] + (hi:lo)   (hi = None: zero-extended lo)"""
    g.I(f"s_add_u32 {sreg(dst)}, {sreg(base)}, {sreg(lo)}")
    g.I(f"s_addc_u32 {sreg(dst + 1)}, {sreg(base + 1)}, {sreg(hi) if hi is not None else 0}")


def gen_tile_bases(g: Gen, c, xdst, wdst, rows_dst, skip_label, full: bool, prefix: str):
    """From S_MT / S_NT: X and W bases and the tile's valid rows into the given registers; full: also every other per-tile scalar of
    the classic kernel's interface (S_Y, S_RES, S_BIAS, S_GATE, S_COLS, S_M0, S_ROWLO, S_LDO) incl. the V-cache redirect.  A V tile
    with nothing to store branches to skip_label.  Scratch: s[56:61], S_T0..2."""
    I = g.I
    m0r, n0 = 56, 57
    I(f"s_lshl_b32 {sreg(m0r)}, {sreg(S_MT)}, 8")
    I(f"s_mul_i32 {sreg(n0)}, {sreg(S_NT)}, {c.WN}")
    I(f"s_mul_i32 {sreg(S_T0)}, {sreg(m0r)}, {sreg(S_LDX)}")
    I(f"s_mul_hi_u32 {sreg(S_T1)}, {sreg(m0r)}, {sreg(S_LDX)}")
    add64(g, xdst, S_XB, S_T0, S_T1)
    I(f"s_mul_i32 {sreg(S_T0)}, {sreg(n0)}, {sreg(S_LDW)}")
    I(f"s_mul_hi_u32 {sreg(S_T1)}, {sreg(n0)}, {sreg(S_LDW)}")
    add64(g, wdst, S_WB, S_T0, S_T1)
    I(f"s_sub_u32 {sreg(rows_dst)}, {sreg(S_MM)}, {sreg(m0r)}")
    if full:
        I(f"s_sub_u32 {sreg(S_COLS)}, {sreg(S_NN)}, {sreg(n0)}")
        I(f"s_mov_b32 {sreg(S_M0)}, {sreg(m0r)}")
        I(f"s_mov_b32 {sreg(S_ROWLO)}, 0")
        I(f"s_mov_b32 {sreg(S_LDO)}, {sreg(S_LDO0)}")
        I(f"s_lshl_b32 {sreg(58)}, {sreg(n0)}, 1")                   # column offset in bytes
        add64(g, S_BIAS, S_BIASB, 58)
        add64(g, S_GATE, S_GATEB, 58)
        I(f"s_mul_i32 {sreg(S_T0)}, {sreg(m0r)}, {sreg(S_LDO0)}")
        I(f"s_mul_hi_u32 {sreg(S_T1)}, {sreg(m0r)}, {sreg(S_LDO0)}")
        I(f"s_add_u32 {sreg(S_T0)}, {sreg(S_T0)}, {sreg(58)}")
        I(f"s_addc_u32 {sreg(S_T1)}, {sreg(S_T1)}, 0")
        add64(g, S_Y, S_YB, S_T0, S_T1)
        add64(g, S_RES, S_RESB, S_T0, S_T1)
    # V tile of the fused QKV projection (gemm_common.h epi_dest): token t -> cache row t + v_shift for v_lo <= t < v_hi
    g.uid += 1
    lab = f"{prefix}_NOTV_{g.uid}"
    I(f"s_cmp_eq_u64 {sreg(S_VOUT, 2)}, 0")
    I(f"s_cbranch_scc1 {lab}")
    I(f"s_cmp_lt_u32 {sreg(n0)}, {sreg(S_VCOL0)}")
    I(f"s_cbranch_scc1 {lab}")
    I(f"s_min_i32 {sreg(59)}, {sreg(S_MM)}, {sreg(S_VHI)}")
    I(f"s_sub_i32 {sreg(59)}, {sreg(59)}, {sreg(m0r)}")              # hi = min(M, v_hi) - m0
    I(f"s_sub_i32 {sreg(60)}, {sreg(S_VLO)}, {sreg(m0r)}")
    I(f"s_max_i32 {sreg(60)}, {sreg(60)}, 0")                        # lo = max(v_lo - m0, 0)
    I(f"s_cmp_le_i32 {sreg(59)}, {sreg(60)}")
    I(f"s_cbranch_scc1 {skip_label}")                                # nothing of this tile is stored
    I(f"s_mov_b32 {sreg(rows_dst)}, {sreg(59)}")
    if full:
        I(f"s_mov_b32 {sreg(S_ROWLO)}, {sreg(60)}")
        I(f"s_mov_b32 {sreg(S_LDO)}, {sreg(S_VC2)}")
        I(f"s_add_i32 {sreg(S_T2)}, {sreg(m0r)}, {sreg(S_VSHIFT)}")  # cache row of the tile's first token (may be negative: rows below lo are not stored)
        I(f"s_mul_i32 {sreg(S_T0)}, {sreg(S_T2)}, {sreg(S_VC2)}")
        I(f"s_mul_hi_i32 {sreg(S_T1)}, {sreg(S_T2)}, {sreg(S_VC2)}")
        I(f"s_sub_u32 {sreg(58)}, {sreg(n0)}, {sreg(S_VCOL0)}")
        I(f"s_lshl_b32 {sreg(58)}, {sreg(58)}, 1")
        I(f"s_add_u32 {sreg(S_T0)}, {sreg(S_T0)}, {sreg(58)}")
        I(f"s_addc_u32 {sreg(S_T1)}, {sreg(S_T1)}, 0")
        add64(g, S_Y, S_VOUT, S_T0, S_T1)
    g.L(lab)


def generate(WN: int, epi: int, prefix: str, i8: bool = False, persistent: bool = False, mfma: int = 32) -> str:
    """Issue order of the staging (one in-order vmcnt queue per wave): W(j) in half-step 2 j - 5, X(j) in half-step 2 j - 4, so at
    the END of the even half-step 2 s the wave has issued ... W(s+1) X(s+1) W(s+2) X(s+2): `s_waitcnt vmcnt(npw + 8)` there = the
    next K-step's operands have landed.  The one barrier per K-step stands right behind that wait: it makes W(s+1) visible (first
    read in half-step 2 s + 1, as the fragments of half-step 2 s + 2) and frees the slot of W(s) (last read in half-step 2 s),
    which the odd half-step then refills with W(s+3).  X needs no barrier: unit (s+1) % 2 is read into FX[(s+1) & 1] in the odd
    half-step of K-step s and refilled (X(s+3)) in the even half-step after it -- the reads are retired by the fragment waits of
    the W reads issued after them (LDS returns in order)."""
    c = Cfg(WN, epi, i8, mfma)
    assert not (persistent and (i8 or epi in (EPI_PARTIAL, EPI_BIAS_SSQ)))
    g = Gen()
    I = g.I
    T = 128                                            # setup scratch (below the address registers, inside the fragment file)
    npw = c.npw
    def ident():
        I(f"v_and_b32 {vreg(c.V_LANE)}, 63, {vreg(V_TID)}")
        I(f"v_lshrrev_b32 {vreg(T)}, 6, {vreg(V_TID)}")
        I("s_nop 0")
        I(f"v_readfirstlane_b32 {sreg(S_WAVE)}, {vreg(T)}")
        I(f"v_and_b32 {vreg(c.V_R)}, 31, {vreg(c.V_LANE)}")
        I(f"v_lshrrev_b32 {vreg(c.V_H)}, 5, {vreg(c.V_LANE)}")
    if persistent:
        ident()                                        # once: v0 (the workitem id) does not survive a tile; V_LANE / V_R / V_H / S_WAVE do
        # ================= tile loop (persistent form): this tile's scalars =================
        I(f"s_mov_b32 {sreg(S_PF)}, 0")
        g.L(f"{prefix}_TILE")
        gen_tile_map(g, S_TILE, T)
        gen_tile_bases(g, c, S_X, S_W, S_ROWS, f"{prefix}_NEXT", True, prefix)
    # ================= setup =================
    if not persistent:
        ident()
    # descriptors: rows bound by num_records (rows past M / N read as zeros), the K offset travels in soffset
    for rs, base, rows, ld in ((S_XRS, S_X, S_ROWS, S_LDX), (S_WRS, S_W, S_COLS, S_LDW)):
        I(f"s_mov_b32 {sreg(rs)}, {sreg(base)}")
        I(f"s_and_b32 {sreg(rs + 1)}, {sreg(base + 1)}, 0xffff")
        I(f"s_min_u32 {sreg(S_T0)}, {sreg(rows)}, 256")
        I(f"s_mul_i32 {sreg(rs + 2)}, {sreg(S_T0)}, {sreg(ld)}")
        I(f"s_mov_b32 {sreg(rs + 3)}, 0x00020000")
    I(f"s_mov_b32 {sreg(S_XK)}, 0")
    I(f"s_mov_b32 {sreg(S_WK)}, 0")
    I(f"s_lshl_b32 {sreg(S_WKMAX)}, {sreg(S_NK)}, 7")                      # S_NK = K / 64 (K-steps)
    I(f"s_sub_u32 {sreg(S_WKMAX)}, {sreg(S_WKMAX)}, 128")
    I(f"s_mov_b32 {sreg(S_XKMAX)}, {sreg(S_WKMAX)}")
    I(f"s_mul_i32 {sreg(S_WM0)}, {sreg(S_WAVE)}, {1024 * npw}")            # this wave's W pieces inside a slot
    I(f"s_mul_i32 {sreg(S_XM0)}, {sreg(S_WAVE)}, {XU * c.xunit}")          # this wave's X units
    I(f"s_add_u32 {sreg(S_XM0)}, {sreg(S_XM0)}, {c.xbase}")
    # DMA source offsets: a piece is 8 rows x 128 B, lane -> row (lane >> 3), LDS position pos = lane & 7 of the row, which
    # fetches source chunk pos ^ ((row >> 1) & 7) (the XOR swizzle is applied on the SOURCE side; the reader undoes it)
    I(f"v_lshrrev_b32 {vreg(T)}, 3, {vreg(c.V_LANE)}")
    I(f"v_and_b32 {vreg(T + 1)}, 7, {vreg(c.V_LANE)}")
    for dst, cnt, ld in ((c.V_DW, npw, S_LDW), (c.V_DX, 8, S_LDX)):
        I(f"s_mul_i32 {sreg(S_T0)}, {sreg(S_WAVE)}, {8 * cnt}")            # first row of this wave's pieces
        for i in range(cnt):
            I(f"v_add_u32 {vreg(T + 2)}, {sreg(S_T0)}, {vreg(T)}")
            I(f"v_add_u32 {vreg(T + 2)}, {8 * i}, {vreg(T + 2)}")          # row within the tile
            I(f"v_lshrrev_b32 {vreg(T + 3)}, 1, {vreg(T + 2)}")
            I(f"v_and_b32 {vreg(T + 3)}, 7, {vreg(T + 3)}")
            I(f"v_xor_b32 {vreg(T + 3)}, {vreg(T + 3)}, {vreg(T + 1)}")
            I(f"v_lshlrev_b32 {vreg(T + 3)}, 4, {vreg(T + 3)}")
            I(f"v_mul_lo_u32 {vreg(dst + i)}, {vreg(T + 2)}, {sreg(ld)}")
            I(f"v_add_u32 {vreg(dst + i)}, {vreg(dst + i)}, {vreg(T + 3)}")
    # rows of this lane (epilogue addressing, idle test)
    I(f"s_lshl_b32 {sreg(S_T0)}, {sreg(S_WAVE)}, 6")                       # 64 w
    for mb in range(c.MB):
        I(f"v_add_u32 {vreg(c.V_ROW + mb)}, {sreg(S_T0)}, {vreg(c.V_R)}")
        if mb:
            I(f"v_add_u32 {vreg(c.V_ROW + mb)}, {32 * mb}, {vreg(c.V_ROW + mb)}")
    # fragment read offsets: row r (+ 32 per block by immediate), chunk at position chunk ^ ((r >> 1) & 7)
    if c.m16:
        # 16-shape: row l & 15 (+ 16 per block by immediate: the swizzle term (row >> 1) & 7 does not see it), chunk 4 hs + (l >> 4)
        I(f"v_and_b32 {vreg(T + 1)}, 15, {vreg(c.V_LANE)}")
        I(f"v_lshrrev_b32 {vreg(T + 3)}, 4, {vreg(c.V_LANE)}")
        I(f"v_lshrrev_b32 {vreg(T)}, 1, {vreg(T + 1)}")
        I(f"v_lshlrev_b32 {vreg(T + 1)}, 7, {vreg(T + 1)}")
    else:
        I(f"v_lshrrev_b32 {vreg(T)}, 1, {vreg(c.V_R)}")
        I(f"v_and_b32 {vreg(T)}, 7, {vreg(T)}")
        I(f"v_lshlrev_b32 {vreg(T + 1)}, 7, {vreg(c.V_R)}")                    # r * 128
    for hs in range(2):
        if c.m16:
            I(f"v_add_u32 {vreg(T + 2)}, {4 * hs}, {vreg(T + 3)}")
            I(f"v_xor_b32 {vreg(T + 2)}, {vreg(T + 2)}, {vreg(T)}")
            I(f"v_lshl_add_u32 {vreg(c.V_WOFF + 2 * hs)}, {vreg(T + 2)}, 4, {vreg(T + 1)}")
            I(f"v_add_u32 {vreg(c.V_WOFF + 4 + 2 * hs)}, 0x10000, {vreg(c.V_WOFF + 2 * hs)}")
            I(f"v_add_u32 {vreg(c.V_WOFF + 8 + 2 * hs)}, 0x20000, {vreg(c.V_WOFF + 2 * hs)}")
            I(f"v_add_u32 {vreg(c.V_XROFF + 2 * hs)}, {sreg(S_XM0)}, {vreg(c.V_WOFF + 2 * hs)}")
            continue
        for ks in range(2):
            I(f"v_add_u32 {vreg(T + 2)}, {4 * hs + 2 * ks}, {vreg(c.V_H)}")
            I(f"v_xor_b32 {vreg(T + 2)}, {vreg(T + 2)}, {vreg(T)}")
            I(f"v_lshl_add_u32 {vreg(c.V_WOFF + 2 * hs + ks)}, {vreg(T + 2)}, 4, {vreg(T + 1)}")
            I(f"v_add_u32 {vreg(c.V_WOFF + 4 + 2 * hs + ks)}, 0x10000, {vreg(c.V_WOFF + 2 * hs + ks)}")
            I(f"v_add_u32 {vreg(c.V_WOFF + 8 + 2 * hs + ks)}, 0x20000, {vreg(c.V_WOFF + 2 * hs + ks)}")
            I(f"v_add_u32 {vreg(c.V_XROFF + 2 * hs + ks)}, {sreg(S_XM0)}, {vreg(c.V_WOFF + 2 * hs + ks)}")     # same row / chunk, own unit
    # prologue staging in the loop's own issue order: W(0) X(0) W(1) X(1) W(2)
    I(f"s_cmp_ge_u32 {sreg(S_T0)}, {sreg(S_ROWS)}")                        # idle waves (their 64 rows are all past M) stage W only
    I(f"s_cbranch_scc1 {prefix}_IDLE")
    n_early = gen_epilogue_setup(g, c)                 # addresses, masks and the early reads of the epilogue (oldest in the queue)
    if persistent:                                     # this tile's first pieces were staged under the previous tile's epilogue
        I(f"s_cmp_eq_u32 {sreg(S_PF)}, 1")
        I(f"s_cbranch_scc1 {prefix}_STAGED")
    for j in range(NSLOT):
        for op in w_dma(c, j):
            I(op)
        if j < XU:
            for op in x_dma(c, j):
                I(op)
    for r in range(c.nacc):                            # accumulators start from zero (while the first tiles fly)
        I(f"v_accvgpr_write_b32 {areg(r)}, 0")
    I(f"s_waitcnt vmcnt({2 * npw + 8})")               # W(0), X(0) have landed
    if persistent:
        I(f"s_branch {prefix}_READY")
        g.L(f"{prefix}_STAGED")
        # the source offsets advance as if the prologue had issued W(0..2), X(0..1) (the prefetch did, from the next-tile bases)
        I(f"s_mov_b32 {sreg(S_WK)}, {128 * NSLOT}")
        I(f"s_min_u32 {sreg(S_WK)}, {sreg(S_WK)}, {sreg(S_WKMAX)}")
        I(f"s_mov_b32 {sreg(S_XK)}, {128 * XU}")
        I(f"s_min_u32 {sreg(S_XK)}, {sreg(S_XK)}, {sreg(S_XKMAX)}")
        for r in range(c.nacc):
            I(f"v_accvgpr_write_b32 {areg(r)}, 0")
        I(f"s_waitcnt vmcnt({n_early})")               # everything older than this tile's early reads: the staged pieces (and the last tile's stores)
        g.L(f"{prefix}_READY")
    I("s_barrier")
    for op in x_frag_reads(c, 0) + w_frag_reads(c, 0):
        I(op)
    I("s_waitcnt lgkmcnt(0)")
    I(f"s_mov_b32 {sreg(S_I)}, 0")
    # ================= main loop over half-steps, unrolled over lcm(NSLOT, XU) K-steps =================
    period = 2 * NSLOT * XU // (2 if NSLOT % 2 == 0 else 1)
    sc = c.sc                                          # the 16-shape has twice the MFMAs (and gaps) per half-step: same fillers, positions scaled
    assert (period // 2) % NSLOT == 0 and (period // 2) % XU == 0
    g.L(f"{prefix}_LOOP")
    for h in range(period):
        s = h >> 1
        mm = mfmas(c, h)
        n = len(mm)
        wr = [] if KN("NO_WREAD") else w_frag_reads(c, h + 1)
        if h & 1 == 0:
            fillers = [(0.6 * sc + k * (n - 6 * sc) / len(wr), op) for k, op in enumerate(wr)] if wr else []
            xd = x_dma(c, s + 2)
            fillers += spread(drop_loads(xd) if KN("NO_X") else xd, 1.3 * sc, n - 1.5 * sc)
            g.phase([] if KN("NO_MFMA") else mm, fillers)
            I(f"s_waitcnt vmcnt({npw + 8})")           # W(s+1), X(s+1) have landed (younger: W(s+2), X(s+2))
            I("s_barrier")                             # W(s+1) visible to all; every wave is done reading the slot of W(s)
        else:
            xr = [] if KN("NO_WREAD") else x_frag_reads(c, s + 1)
            fillers = [((0.3 + k * 0.5) * sc, op) for k, op in enumerate(xr)]            # ahead of the W reads: retired with them
            fillers += [(4.6 * sc + k * (n - 10 * sc) / len(wr), op) for k, op in enumerate(wr)] if wr else []
            wd = w_dma(c, s + 3)
            fillers += spread(drop_loads(wd) if KN("NO_W") else wd, 1.3 * sc, n - 1.5 * sc)
            g.phase([] if KN("NO_MFMA") else mm, fillers)
            I(f"s_add_u32 {sreg(S_I)}, {sreg(S_I)}, 1")
            I(f"s_cmp_ge_u32 {sreg(S_I)}, {sreg(S_NK)}")
            I(f"s_cbranch_scc1 {prefix}_EPI")
    I(f"s_branch {prefix}_LOOP")
    # ================= epilogue =================
    g.L(f"{prefix}_EPI")
    I("s_nop 15")
    I("s_nop 15")
    if KN("NO_EPI") and not persistent:
        I("s_waitcnt vmcnt(0)")
        I("s_endpgm")
    if persistent:
        gen_prefetch(g, c, prefix, "A")                # (older than every operation the epilogue issues: its counted waits are unaffected)
    tail_stores = 0 if KN("NO_EPI") else gen_epilogue(g, c)      # (timing-only: the persistent form keeps its tile walk without the epilogue)
    if persistent:
        g.L(f"{prefix}_NEXT")                          # (also the target of a V tile that stores nothing)
        I(f"s_add_u32 {sreg(S_TILE)}, {sreg(S_TILE)}, {sreg(S_GRID)}")
        I(f"s_cmp_lt_u32 {sreg(S_TILE)}, {sreg(S_NTILES)}")
        I(f"s_cbranch_scc1 {prefix}_TILE")
    # every load of the wave (the over-run staging pieces included: they are older) has landed once at most the epilogue's trailing
    # stores are outstanding; the wave does not wait for those to be acknowledged
    I(f"s_waitcnt vmcnt({0 if persistent else min(63, tail_stores)})")
    I("s_endpgm")
    # ================= idle waves: their share of W, the barriers =================
    g.L(f"{prefix}_IDLE")
    if persistent:
        I(f"s_cmp_eq_u32 {sreg(S_PF)}, 1")
        I(f"s_cbranch_scc1 {prefix}_IDLE_STAGED")
    for j in range(NSLOT):
        for op in w_dma(c, j):
            I(op)
    I(f"s_waitcnt vmcnt({2 * npw})")
    if persistent:
        I(f"s_branch {prefix}_IDLE_READY")
        g.L(f"{prefix}_IDLE_STAGED")
        I(f"s_mov_b32 {sreg(S_WK)}, {128 * NSLOT}")
        I(f"s_min_u32 {sreg(S_WK)}, {sreg(S_WK)}, {sreg(S_WKMAX)}")
        I("s_waitcnt vmcnt(0)")
        g.L(f"{prefix}_IDLE_READY")
    I("s_barrier")
    I(f"s_mov_b32 {sreg(S_I)}, 0")
    g.L(f"{prefix}_IDLE_LOOP")
    for st in range(NSLOT):
        I(f"s_waitcnt vmcnt({npw})")
        I("s_barrier")
        for op in w_dma(c, st + 3):
            I(op)
        I(f"s_add_u32 {sreg(S_I)}, {sreg(S_I)}, 1")
        I(f"s_cmp_ge_u32 {sreg(S_I)}, {sreg(S_NK)}")
        I(f"s_cbranch_scc1 {prefix}_IDLE_END")
    I(f"s_branch {prefix}_IDLE_LOOP")
    g.L(f"{prefix}_IDLE_END")
    if persistent:
        gen_prefetch(g, c, prefix, "I")                # the barrier all waves share + this wave's share of the next tile's first pieces
        I(f"s_branch {prefix}_NEXT")
    else:
        I("s_waitcnt vmcnt(0)")
        I("s_endpgm")
    return finalize(g.out)


def gen_prefetch(g: Gen, c: Cfg, prefix: str, tag: str):
    """Persistent form, at the end of a tile's loop: one barrier (every wave is done reading the W slots), then the NEXT tile of this
    workgroup is mapped and -- unless there is none, or it is a V tile that stores nothing -- its W(0..2) and, for waves that have
    rows in it, X(0..1) are issued; S_PF says so to the next tile's prologue.  These operations are OLDER than anything the epilogue
    issues, so its counted waits (which count younger operations) stand as they are."""
    I = g.I
    T = 128
    npw = c.npw
    I("s_barrier")
    I(f"s_mov_b32 {sreg(S_PF)}, 0")
    I(f"s_add_u32 {sreg(S_I)}, {sreg(S_TILE)}, {sreg(S_GRID)}")     # (the loop counter is dead here)
    I(f"s_cmp_ge_u32 {sreg(S_I)}, {sreg(S_NTILES)}")
    I(f"s_cbranch_scc1 {prefix}_PF_DONE_{tag}")
    gen_tile_map(g, S_I, T)
    gen_tile_bases(g, c, S_XN, S_WN, S_ROWSN, f"{prefix}_PF_DONE_{tag}", False, prefix)
    I(f"s_mov_b32 {sreg(S_PF)}, 1")
    # descriptors of the next tile (rows bound as in the setup), K offsets from zero
    for rs, base, rows, ld in ((S_WRS, S_WN, None, S_LDW), (S_XRS, S_XN, S_ROWSN, S_LDX)):
        I(f"s_mov_b32 {sreg(rs)}, {sreg(base)}")
        I(f"s_and_b32 {sreg(rs + 1)}, {sreg(base + 1)}, 0xffff")
        if rows is None:                               # N - n0 of the next tile, >= WN on this path: all WN rows of W are valid
            I(f"s_mul_i32 {sreg(rs + 2)}, {sreg(ld)}, {c.WN}")
        else:
            I(f"s_min_u32 {sreg(S_T0)}, {sreg(rows)}, 256")
            I(f"s_mul_i32 {sreg(rs + 2)}, {sreg(S_T0)}, {sreg(ld)}")
        I(f"s_mov_b32 {sreg(rs + 3)}, 0x00020000")
    I(f"s_mov_b32 {sreg(S_XK)}, 0")
    I(f"s_mov_b32 {sreg(S_WK)}, 0")
    I(f"s_lshl_b32 {sreg(S_T0)}, {sreg(S_WAVE)}, 6")
    I(f"s_cmp_ge_u32 {sreg(S_T0)}, {sreg(S_ROWSN)}")                # this wave has no rows in the next tile: W only
    I(f"s_cbranch_scc1 {prefix}_PF_WONLY_{tag}")
    for j in range(NSLOT):
        for op in w_dma(c, j):
            I(op)
        if j < XU:
            for op in x_dma(c, j):
                I(op)
    I(f"s_branch {prefix}_PF_DONE_{tag}")
    g.L(f"{prefix}_PF_WONLY_{tag}")
    for j in range(NSLOT):
        for op in w_dma(c, j):
            I(op)
    g.L(f"{prefix}_PF_DONE_{tag}")



def gen_epilogue_setup(g: Gen, c: Cfg):
    """Before the loop (active waves): the epilogue's addresses and masks, and its early reads (the OLDEST entries of the wave's
    vmcnt queue: every later wait covers them)."""
    I = g.I
    T = c.V_T
    epi = c.epi
    EA = c.V_EA
    # row addressing: byte offset of the lane's row in Y / RES: row * ldo + 16 h (the swap gives the upper half the second 16 bytes)
    for mb in range(c.MB):
        I(f"v_mul_lo_u32 {vreg(EA + mb)}, {vreg(c.V_ROW + mb)}, {sreg(S_LDO)}")
        I(f"v_lshl_add_u32 {vreg(EA + mb)}, {vreg(c.V_H)}, 4, {vreg(EA + mb)}")
    # 16-shape: BEFORE the lane exchange a lane holds rows 16 mb16 + (l & 15) and, per 16-column block, columns 4 q + (0..3), q = l >> 4;
    # AFTER it (v_permlane16_swap between the two 16-row blocks of a 32-row block) the same rows and 16-byte column runs as the
    # 32-shape after its swap -- row 32 mb + (l & 31), columns 8 h + (0..7) per 16-column block -- so everything above is shared
    R16, Q16 = T + 60, T + 61
    if c.m16:
        I(f"v_and_b32 {vreg(R16)}, 0xffffffef, {vreg(c.V_ROW)}")             # 64 w + (l & 15)
        I(f"v_lshrrev_b32 {vreg(Q16)}, 4, {vreg(c.V_LANE)}")
        I(f"v_lshlrev_b32 {vreg(EA + 2)}, 3, {vreg(Q16)}")                   # bias / gate column byte offset of this lane group: 8 q
    else:
        I(f"v_lshlrev_b32 {vreg(EA + 2)}, 3, {vreg(c.V_H)}")                     # bias / gate column byte offset of this half: 8 h
    if epi == EPI_GATE_RES:
        # gate row of the lane's row: frame = (m0 + row) / frame_len  (integer division via float with one correction each way)
        I(f"s_sub_u32 {sreg(S_T1)}, {sreg(S_ROWS)}, 1")                      # rows past M take the last valid row's frame (gemm_common.h: mc = min(m, M - 1)):
        for mb in range(4 if c.m16 else c.MB):                               # their gate address must stay inside the table
            m, q, t = T + 66, EA + 3 + mb, T + 48
            if c.m16:                                                        # (mb counts 16-row blocks here)
                I(f"v_add_u32 {vreg(m)}, {16 * mb}, {vreg(R16)}")
                I(f"v_min_u32 {vreg(m)}, {sreg(S_T1)}, {vreg(m)}")
            else:
                I(f"v_min_u32 {vreg(m)}, {sreg(S_T1)}, {vreg(c.V_ROW + mb)}")
            I(f"v_add_u32 {vreg(m)}, {sreg(S_M0)}, {vreg(m)}")
            I(f"v_cvt_f32_u32 {vreg(t)}, {vreg(m)}")
            I(f"v_cvt_f32_u32 {vreg(t + 1)}, {sreg(S_FLEN)}")
            I(f"v_rcp_f32 {vreg(t + 1)}, {vreg(t + 1)}")
            I("s_nop 0")
            I(f"v_mul_f32 {vreg(t)}, {vreg(t)}, {vreg(t + 1)}")
            I(f"v_cvt_u32_f32 {vreg(q)}, {vreg(t)}")                         # q ~ m / flen (may be one off)
            I(f"v_mul_lo_u32 {vreg(t)}, {vreg(q)}, {sreg(S_FLEN)}")          # q * flen
            I(f"v_cmp_gt_u32_e64 {sreg(S_MSK, 2)}, {vreg(t)}, {vreg(m)}")    # too big -> q - 1
            I(f"v_cndmask_b32_e64 {vreg(t + 2)}, 0, 1, {sreg(S_MSK, 2)}")
            I(f"v_sub_u32 {vreg(q)}, {vreg(q)}, {vreg(t + 2)}")
            I(f"v_mul_lo_u32 {vreg(t)}, {vreg(q)}, {sreg(S_FLEN)}")
            I(f"v_add_u32 {vreg(t)}, {sreg(S_FLEN)}, {vreg(t)}")             # (q + 1) * flen <= m -> q + 1
            I(f"v_cmp_le_u32_e64 {sreg(S_MSK, 2)}, {vreg(t)}, {vreg(m)}")
            I(f"v_cndmask_b32_e64 {vreg(t + 2)}, 0, 1, {sreg(S_MSK, 2)}")
            I(f"v_add_u32 {vreg(q)}, {vreg(q)}, {vreg(t + 2)}")
            I(f"v_mul_lo_u32 {vreg(q)}, {vreg(q)}, {sreg(S_GSTRIDE)}")       # byte offset of the frame's gate row
            I(f"v_lshl_add_u32 {vreg(q)}, {vreg(Q16 if c.m16 else c.V_H)}, 3, {vreg(q)}")      # + 8 h: the gate is applied in the accumulator layout (as the bias)
    for mb in range(c.MB):                                                   # stored rows: row_lo <= row < rows
        I(f"v_cmp_lt_u32_e64 {sreg(S_MSK + 2 * mb, 2)}, {vreg(c.V_ROW + mb)}, {sreg(S_ROWS)}")
        I(f"v_cmp_ge_u32_e64 vcc, {vreg(c.V_ROW + mb)}, {sreg(S_ROWLO)}")
        I(f"s_and_b64 {sreg(S_MSK + 2 * mb, 2)}, {sreg(S_MSK + 2 * mb, 2)}, vcc")
    if c.i8:
        # W8A8: the lane's activation scale per row block (rows past M: the last valid row's, never stored) and the byte offset of
        # its four weight-scale columns inside a 32-column block
        I(f"v_lshlrev_b32 {vreg(EA + 5)}, 4, {vreg(c.V_H)}")
        I(f"s_sub_u32 {sreg(S_T1)}, {sreg(S_ROWS)}, 1")
        for mb in range(c.MB):
            I(f"v_min_u32 {vreg(T + 48)}, {sreg(S_T1)}, {vreg(c.V_ROW + mb)}")
            I(f"v_lshlrev_b32 {vreg(T + 48)}, 2, {vreg(T + 48)}")
            I(f"global_load_dword {vreg(c.V_SX + 2 * mb)}, {vreg(T + 48)}, {sreg(S_SX, 2)}")
    # early reads
    n0 = sum(1 for l in g.out if l.startswith("global_load"))
    for nb in range(c.early_nb):
        for g4 in range(c.bl):                                                # (16-shape: g4 = the 16-column half of the block)
            I(f"global_load_dwordx2 {vreg(c.V_EB + 8 * nb + 2 * g4, 2)}, {vreg(EA + 2)}, {sreg(S_BIAS, 2)} offset:{64 * nb + (64 // c.bl) * g4}")
    if c.nl:
        epi_block_loads(g, c, 0, c.V_E0)
    return sum(1 for l in g.out if l.startswith("global_load")) - n0 + (c.MB if c.i8 else 0)      # vector-memory reads issued here


def epi_block_loads(g: Gen, c: Cfg, j: int, P: int):
    """gate / residual pieces of epilogue block j = (nb, mb) into P[0:16]"""
    I = g.I
    nb, mb = j // c.MB, j % c.MB
    EA = c.V_EA
    if c.epi == EPI_GATE_RES:                                                # gate[frame][n] in the accumulator layout (as the bias)
        for g4 in range(4):
            if c.m16:                                                        # group g4 = (16-column half g4 >> 1, 16-row half g4 & 1) of the block
                I(f"global_load_dwordx2 {vreg(P + 2 * g4, 2)}, {vreg(EA + 3 + 2 * mb + (g4 & 1))}, {sreg(S_GATE, 2)} offset:{64 * nb + 32 * (g4 >> 1)}")
                continue
            I(f"global_load_dwordx2 {vreg(P + 2 * g4, 2)}, {vreg(EA + 3 + mb)}, {sreg(S_GATE, 2)} offset:{64 * nb + 16 * g4}")
    if c.epi in (EPI_GATE_RES, EPI_RES):                                     # residual in the 8-column layout after the swap
        I(f"s_mov_b64 exec, {sreg(S_MSK + 2 * mb, 2)}")
        for k in (0, 2):
            I(f"global_load_dwordx4 {vreg(P + 8 + 2 * k, 4)}, {vreg(EA + mb)}, {sreg(S_RES, 2)} offset:{64 * nb + 16 * k}")
        I("s_mov_b64 exec, -1")


def gen_epilogue(g: Gen, c: Cfg):
    """per (mb, nb): 16 accumulators of a lane = its row m, columns 32 nb + 8 g4 + 4 h + (0..3), g4 = 0..3.
    16-shape: the block (mb, nb) is the four 16 x 16 tiles (mb16, nb16) = (2 mb + a, 2 nb + cc); group g4 = 2 cc + a of the lane's 16
    values is row 32 mb + 16 a + (l & 15), columns 32 nb + 16 cc + 4 q + (0..3), q = l >> 4.  v_permlane16_swap between the groups
    a = 0 / 1 of one cc (the 16-lane analogue of T21) leaves every lane with the 16-byte runs of the 32-shape after its swap, so the
    residual arithmetic, the row masks and the stores are the same text; the rounding points and their order are untouched."""
    I = g.I
    T = c.V_T
    epi = c.epi
    EA = c.V_EA
    K0, K1, CEXP = 0.7978845608028654, 0.044715, -2.0 * 1.4426950408889634
    # constants in SGPR pairs for the packed ops
    cons = {}
    def const_pair(name, val, s0):
        I(f"s_mov_b32 {sreg(s0)}, {hex(f32bits(val))}")
        I(f"s_mov_b32 {sreg(s0 + 1)}, {hex(f32bits(val))}")
        cons[name] = s0
    if epi == EPI_GELU:
        const_pair("k1", K1, 54); const_pair("k0", K0, 56); const_pair("ce", CEXP, 58); const_pair("one", 1.0, 60)
    if epi == EPI_BIAS_SSQ:
        for k in range((4 if c.m16 else 2) * c.MB):
            I(f"v_mov_b32 {vreg(c.V_SS + k)}, 0")
    if epi == EPI_PARTIAL:
        # fp32 accumulators as they stand: a lane owns row m, columns 32 nb + 8 g4 + 4 h + (0..3) = 16 contiguous bytes per group
        for nb in range(c.NB):
            for mb in range(c.MB):
                a0 = c.acc(mb, nb)
                for r in range(16):
                    I(f"v_accvgpr_read_b32 {vreg(T + r)}, {areg(a0 + r)}")
                I(f"s_mov_b64 exec, {sreg(S_MSK + 2 * mb, 2)}")
                for g4 in range(4):
                    I(f"global_store_dwordx4 {vreg(EA + mb)}, {vreg(T + 4 * g4, 4)}, {sreg(S_Y, 2)} offset:{128 * nb + 32 * g4}")
                I("s_mov_b64 exec, -1")
        return 4 * c.NB * c.MB
    # Every global read of the epilogue is issued ahead of its use: the early ones before the loop (gen_epilogue_setup), here the
    # bias vectors that did not fit up there, then the gate / residual pieces of block j + 1 while block j computes.
    BB, PB = T + 72, T + 72 + 8 * c.NB                                       # late bias raw [nb][g4] (2 registers each); block buffers P[2][16]
    assert PB + 32 <= min(c.V_WOFF + 32, 256), (PB, c.V_WOFF)               # below the registers that survive the loop (V_LANE ...)
    n_late = c.bl * (c.NB - c.early_nb)
    q = []                                                                   # vector-memory operations issued by the epilogue, in order
    SWB = PB + 32                                                            # W8A8: weight scales of the current / next column block, 2 x 16 registers
    assert not c.i8 or SWB + 32 <= c.V_LANE, (SWB, c.V_LANE)

    def wait_for(tags):
        """vmcnt that retires every operation carrying one of `tags` (None: none of them was issued here)"""
        idx = [i for i, t in enumerate(q) if t in tags]
        return None if not idx else min(63, len(q) - 1 - idx[-1])

    def sw_loads(nb):
        for g4 in range(4):
            I(f"global_load_dwordx4 {vreg(SWB + 16 * (nb & 1) + 4 * g4, 4)}, {vreg(EA + 5)}, {sreg(S_SW, 2)} offset:{128 * nb + 32 * g4}")
        q.extend([("sw", nb)] * 4)

    for nb in range(c.early_nb, c.NB):                                       # lane needs columns 32 nb + 8 g4 + 4 h + (0..3): 4 loads of 8 bytes
        for g4 in range(c.bl):                                               # (16-shape: columns 32 nb + 16 g4 + 4 q + (0..3): 2 loads)
            I(f"global_load_dwordx2 {vreg(BB + 8 * nb + 2 * g4, 2)}, {vreg(EA + 2)}, {sreg(S_BIAS, 2)} offset:{64 * nb + (64 // c.bl) * g4}")
        q.extend([("bias", nb)] * c.bl)
    if c.i8:
        sw_loads(0)
        for mb in range(c.MB):                                               # (sx, sx) pairs for the packed multiplies
            I(f"v_mov_b32 {vreg(c.V_SX + 2 * mb + 1)}, {vreg(c.V_SX + 2 * mb)}")
    blocks = [(nb, mb) for nb in range(c.NB) for mb in range(c.MB)]
    nl = c.nl

    for j, (nb, mb) in enumerate(blocks):
        P = c.V_E0 if j == 0 else PB + 16 * (j & 1)
        if c.i8 and mb == 0 and nb + 1 < c.NB:
            sw_loads(nb + 1)
        if nl and j + 1 < len(blocks):
            epi_block_loads(g, c, j + 1, PB + 16 * ((j + 1) & 1))
            q.extend([("blk", j + 1)] * nl)
        nxt_loads = nl if (nl and j + 1 < len(blocks)) else 0
        if c.i8:                                                             # waits counted from the issue order
            need = [("blk", j)] + ([("bias", nb), ("sw", nb)] if mb == 0 else [])
            n = wait_for(need)
            if n is not None:
                I(f"s_waitcnt vmcnt({n})")
        elif nl and j == 0:
            I(f"s_waitcnt vmcnt({(n_late if c.early_nb else 0) + nxt_loads})")   # block 0's pieces are early; its bias vector is late only when none fit up there
        elif nl:                                                             # younger than block j's loads: block j-1's two stores, block j+1's loads
            I(f"s_waitcnt vmcnt({2 + nxt_loads})")
        elif c.early_nb == 0 and j == 0:
            I("s_waitcnt vmcnt(0)")                                          # the bias vectors
        if not nl and mb == 0 and nb == c.early_nb and 0 < c.early_nb < c.NB:
            I(f"s_waitcnt vmcnt({min(63, 2 * j)})")                          # the late bias vectors (younger: the stores so far)
        if mb == 0:
            for g4 in range(4):                                              # bf16 x4 -> f32 x4: T+24+4 g4 .. +3
                for d in range(2):
                    src = (c.V_EB if nb < c.early_nb else BB) + 8 * nb + 2 * (g4 >> 1 if c.m16 else g4) + d
                    I(f"v_lshlrev_b32 {vreg(T + 24 + 4 * g4 + 2 * d)}, 16, {vreg(src)}")
                    I(f"v_and_b32 {vreg(T + 24 + 4 * g4 + 2 * d + 1)}, 0xffff0000, {vreg(src)}")
        a0 = c.acc(mb, nb)
        # v = bf16(acc + bias), kept as f32 in T+0..15
        for r in range(16):
            src = c.acc16(2 * mb + ((r >> 2) & 1), 2 * nb + (r >> 3)) + (r & 3) if c.m16 else a0 + r
            I(f"v_accvgpr_read_b32 {vreg(T + r)}, {areg(src)}")
        if c.i8:                                                             # acc_f * (sx[m] * sw[n]) with gemm_common.h's order of operations
            for r in range(16):
                I(f"v_cvt_f32_i32 {vreg(T + r)}, {vreg(T + r)}")
            for r in range(0, 16, 2):
                I(f"v_pk_mul_f32 {vreg(T + 56, 2)}, {vreg(SWB + 16 * (nb & 1) + r, 2)}, {vreg(c.V_SX + 2 * mb, 2)}")
                I(f"v_pk_mul_f32 {vreg(T + r, 2)}, {vreg(T + r, 2)}, {vreg(T + 56, 2)}")
        for r in range(0, 16, 2):
            I(f"v_pk_add_f32 {vreg(T + r, 2)}, {vreg(T + r, 2)}, {vreg(T + 24 + r, 2)}")
        for r in range(0, 16, 2):                                            # round to bf16 and back
            I(f"v_cvt_pk_bf16_f32 {vreg(T + 16 + r // 2)}, {vreg(T + r)}, {vreg(T + r + 1)}")
        if epi in (EPI_GELU, EPI_GATE_RES, EPI_BIAS_SSQ):
            for r in range(0, 16, 2):
                I(f"v_lshlrev_b32 {vreg(T + r)}, 16, {vreg(T + 16 + r // 2)}")
                I(f"v_and_b32 {vreg(T + r + 1)}, 0xffff0000, {vreg(T + 16 + r // 2)}")
        if epi == EPI_BIAS_SSQ:                                              # SS[mb] += v * v of the ROUNDED outputs, fixed order: nb, then the 8 pairs
            for r in range(0, 16, 2):                                        # (16-shape: SS[mb16] of the group's row half)
                ss = c.V_SS + 2 * (2 * mb + ((r >> 2) & 1) if c.m16 else mb)
                I(f"v_pk_fma_f32 {vreg(ss, 2)}, {vreg(T + r, 2)}, {vreg(T + r, 2)}, {vreg(ss, 2)}")
        if epi == EPI_GATE_RES:                                              # w = bf16(v * gate[frame][n])
            for r in range(0, 16, 2):
                src = P + r // 2
                I(f"v_lshlrev_b32 {vreg(T + 56)}, 16, {vreg(src)}")
                I(f"v_and_b32 {vreg(T + 57)}, 0xffff0000, {vreg(src)}")
                I(f"v_pk_mul_f32 {vreg(T + r, 2)}, {vreg(T + r, 2)}, {vreg(T + 56, 2)}")
            for r in range(0, 16, 2):
                I(f"v_cvt_pk_bf16_f32 {vreg(T + 16 + r // 2)}, {vreg(T + r)}, {vreg(T + r + 1)}")
        if epi == EPI_GELU:
            # y = x * rcp(1 + exp2(ce * (k0 * (x + ((k1 * x) * x) * x))))   (gemm_common.h / common.h gelu_tanh, contraction off)
            for r in range(0, 16, 2):
                x, t = vreg(T + r, 2), vreg(T + 44 + (r % 4), 2)
                I(f"v_pk_mul_f32 {t}, {sreg(cons['k1'], 2)}, {x}")
                I(f"v_pk_mul_f32 {t}, {t}, {x}")
                I(f"v_pk_mul_f32 {t}, {t}, {x}")
                I(f"v_pk_add_f32 {t}, {x}, {t}")
                I(f"v_pk_mul_f32 {t}, {sreg(cons['k0'], 2)}, {t}")
                I(f"v_pk_mul_f32 {t}, {sreg(cons['ce'], 2)}, {t}")
                I(f"v_exp_f32 {vreg(T + 44 + (r % 4))}, {vreg(T + 44 + (r % 4))}")
                I(f"v_exp_f32 {vreg(T + 45 + (r % 4))}, {vreg(T + 45 + (r % 4))}")
                I("s_nop 0")                                                 # transcendental result -> VALU: one wait state
                I(f"v_pk_add_f32 {t}, {sreg(cons['one'], 2)}, {t}")
                I(f"v_rcp_f32 {vreg(T + 44 + (r % 4))}, {vreg(T + 44 + (r % 4))}")
                I(f"v_rcp_f32 {vreg(T + 45 + (r % 4))}, {vreg(T + 45 + (r % 4))}")
                I("s_nop 0")
                I(f"v_pk_mul_f32 {x}, {x}, {t}")
            for r in range(0, 16, 2):
                I(f"v_cvt_pk_bf16_f32 {vreg(T + 16 + r // 2)}, {vreg(T + r)}, {vreg(T + r + 1)}")
        # packed bf16 in T+16..23: dwords (2 g4, 2 g4 + 1) = columns 8 g4 + 4 h + (0..3).  T21: swap pairs (g4 = 0,1) and (2,3)
        for k in (0, 2):
            ax, ay, bx, by = T + 16 + 2 * k, T + 17 + 2 * k, T + 18 + 2 * k, T + 19 + 2 * k
            I("s_nop 1")
            swap = "v_permlane16_swap_b32" if c.m16 else "v_permlane32_swap_b32"          # 16-shape: groups (cc, a = 0) and (cc, a = 1), cc = k / 2
            I(f"{swap} {vreg(ax)}, {vreg(bx)}")
            I(f"{swap} {vreg(ay)}, {vreg(by)}")
        off_y = 64 * nb
        if epi in (EPI_GATE_RES, EPI_RES):
            # residual arithmetic in the 8-column layout after the swap: out = bf16(res + w), w = v or bf16(v * gate)
            for k in (0, 2):
                for d in range(4):                                           # 8 columns: res + v in f32, rounded once
                    vsrc, rsrc = T + 16 + 2 * k + d, P + 8 + 2 * k + d
                    I(f"v_lshlrev_b32 {vreg(T)}, 16, {vreg(vsrc)}")
                    I(f"v_and_b32 {vreg(T + 1)}, 0xffff0000, {vreg(vsrc)}")
                    I(f"v_lshlrev_b32 {vreg(T + 2)}, 16, {vreg(rsrc)}")
                    I(f"v_and_b32 {vreg(T + 3)}, 0xffff0000, {vreg(rsrc)}")
                    I(f"v_pk_add_f32 {vreg(T, 2)}, {vreg(T + 2, 2)}, {vreg(T, 2)}")
                    I(f"v_cvt_pk_bf16_f32 {vreg(vsrc)}, {vreg(T)}, {vreg(T + 1)}")
        I(f"s_mov_b64 exec, {sreg(S_MSK + 2 * mb, 2)}")
        for k in (0, 2):
            I(f"global_store_dwordx4 {vreg(EA + mb)}, {vreg(T + 16 + 2 * k, 4)}, {sreg(S_Y, 2)} offset:{off_y + 16 * k}")
        I("s_mov_b64 exec, -1")
        q.extend([("st", j)] * 2)
    if epi == EPI_BIAS_SSQ and c.m16:
        # row sum of the tile, fixed order: per lane group q the pairs in the order above, even + odd columns; then (q0 + q2) + (q1 + q3)
        # (lanes l, l + 16, l + 32, l + 48 hold the four column quarters of row 16 mb16 + (l & 15)); one 4-byte store per valid row
        # from lane group 0
        R16, Q16 = T + 8, T + 9
        I(f"v_and_b32 {vreg(R16)}, 0xffffffef, {vreg(c.V_ROW)}")             # 64 w + (l & 15)
        I(f"v_lshrrev_b32 {vreg(Q16)}, 4, {vreg(c.V_LANE)}")
        for step in ("v_permlane32_swap_b32", "v_permlane16_swap_b32"):
            for mb in range(4):
                ss = c.V_SS + 2 * mb
                I(f"v_add_f32 {vreg(ss)}, {vreg(ss)}, {vreg(ss + 1)}")
                I(f"v_mov_b32 {vreg(ss + 1)}, {vreg(ss)}")
            I("s_nop 1")
            for mb in range(4):
                ss = c.V_SS + 2 * mb
                I(f"{step} {vreg(ss)}, {vreg(ss + 1)}")                      # ss = the lower group's sum in both groups, ss + 1 = the upper group's
        for mb in range(4):
            ss = c.V_SS + 2 * mb
            I(f"v_add_f32 {vreg(ss)}, {vreg(ss)}, {vreg(ss + 1)}")
            I(f"v_add_u32 {vreg(T + mb)}, {16 * mb}, {vreg(R16)}")                      # the row
            I(f"v_cmp_lt_u32_e64 vcc, {vreg(T + mb)}, {sreg(S_ROWS)}")
            I(f"v_cmp_eq_u32_e64 {sreg(S_MT, 2)}, {vreg(Q16)}, 0")           # (s[54:55]: free in the classic form)
            I(f"s_and_b64 vcc, vcc, {sreg(S_MT, 2)}")
            I(f"v_lshlrev_b32 {vreg(T + mb)}, 2, {vreg(T + mb)}")                       # byte offset of the row's sum
            I("s_mov_b64 exec, vcc")
            I(f"global_store_dword {vreg(T + mb)}, {vreg(ss)}, {sreg(S_SSQ, 2)}")
            I("s_mov_b64 exec, -1")
            q.append(("st", "ssq"))
    elif epi == EPI_BIAS_SSQ:
        # row sum of the tile: (even + odd columns) of this half, + the other half of the wave (lanes r and r + 32 hold the two
        # halves of row r's columns); one 4-byte store per valid row from the lower half
        for mb in range(c.MB):
            ss = c.V_SS + 2 * mb
            I(f"v_add_f32 {vreg(ss)}, {vreg(ss)}, {vreg(ss + 1)}")
            I(f"v_mov_b32 {vreg(ss + 1)}, {vreg(ss)}")
        I("s_nop 1")
        for mb in range(c.MB):
            ss = c.V_SS + 2 * mb
            I(f"v_permlane32_swap_b32 {vreg(ss)}, {vreg(ss + 1)}")          # ss = (lower, lower), ss + 1 = (upper, upper)
        for mb in range(c.MB):
            ss = c.V_SS + 2 * mb
            I(f"v_add_f32 {vreg(ss)}, {vreg(ss)}, {vreg(ss + 1)}")
            I(f"v_lshlrev_b32 {vreg(T + mb)}, 2, {vreg(c.V_ROW + mb)}")                 # byte offset of the row's sum
            I(f"v_cmp_eq_u32_e64 vcc, {vreg(c.V_H)}, 0")
            I(f"s_and_b64 vcc, vcc, {sreg(S_MSK + 2 * mb, 2)}")
            I("s_mov_b64 exec, vcc")
            I(f"global_store_dword {vreg(T + mb)}, {vreg(ss)}, {sreg(S_SSQ, 2)}")
            I("s_mov_b64 exec, -1")
            q.append(("st", "ssq"))
    n = 0
    while n < len(q) and q[len(q) - 1 - n][0] == "st":
        n += 1
    return n


if __name__ == "__main__":
    if "--diag" in sys.argv:
        sys.argv.remove("--diag")                                            # (attn_asm_gen saw it at import: timing-only knobs allowed)
    WN, epi = int(sys.argv[1]), int(sys.argv[2])
    form = sys.argv[5] if len(sys.argv) > 5 else ""                          # "", "i8", "p" (persistent), "m16" / "pm16" (16x16x32 MFMA shape)
    i8, pers, mfma = form == "i8", form in ("p", "pm16"), 16 if form in ("m16", "pm16") else 32
    txt = generate(WN, epi, f"GA{WN}E{epi}" + ("I8" if i8 else "") + ("P" if pers else "") + ("M16" if mfma == 16 else ""), i8, pers, mfma)
    probs = lint(txt)
    for p in probs[:20]:
        print("LINT:", p, file=sys.stderr)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(to_inc(txt))
    if len(sys.argv) > 4:
        open(sys.argv[4], "w").write(txt)
    n = sum(1 for l in txt.splitlines() if l and not l.endswith(":"))
    print(f"gemm WN={WN} epi={epi}: {n} instructions, {len(probs)} lint findings", file=sys.stderr)
    sys.exit(1 if probs else 0)
