"""Host side of the code-emitting attention edge suite (tests/attn_qout_exact.py; the GPU side is tests/test_attn_qout_edges_gpu.py).

For every geometry and format the picked-row construction's own conditions hold on the CPU, so that its expected bytes need no
kernel: every other in-range key trails the picked one by more than 150 binary orders, the first and the last slot of the range are
picked, every slot outside the range is a decoy that would change a row's bytes if admitted.  The expected bytes contain what the
suite is there for (an all-zero block, a clamped exponent, edge blocks on rows of the first and last wave of the last workgroup in
both halves, heads that differ).  Where one workgroup covers the geometry, the generated text of each format runs on the CPU
emulator and the WHOLE sentinel-filled code and scale buffers equal the expected ones."""
import numpy as np
import pytest
import torch

import attn_qout_exact as Q
from attn_qout_emu import BITS, G, QUANT, SENT, expected, head_code_bytes, run

ALL = [(g, f) for g in Q.QOUT_ASM_CASES for f in Q.FMTS] + [(g, "mx") for g in Q.QOUT_ASM_ODD]
_ids = lambda v: Q.case_id(v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def texts():
    return {f: G.generate("buffer", "LLB" + f.upper(), out=f) for f in Q.FMTS}


def block_bytes(fmt, h, db):
    """byte positions, inside a packed row, of block db of head h"""
    return head_code_bytes(fmt, h).reshape(4, -1)[db]


def test_the_geometry_list_is_the_bf16_suites_with_even_heads():
    import bf16_exact
    assert [(B, Lq, rg) for B, Lq, _, rg in Q.QOUT_ASM_CASES[:12]] == [(B, Lq, rg) for B, Lq, _, rg in bf16_exact.ASM_CASES]
    assert [H for _, _, H, _ in Q.QOUT_ASM_CASES] == [2, 2, 4, 2, 2, 4, 2, 4, 2, 12, 2, 4, 2, 4]
    assert sorted({Lq for _, Lq, _, _ in Q.QOUT_ASM_CASES}) == [1, 31, 32, 33, 64, 127, 128, 129, 255, 256, 257, 328]
    assert {(Lq, H) for _, Lq, H, _ in Q.QOUT_ASM_ODD} == {(33, 1), (33, 3), (257, 1), (257, 3)}
    # waves with valid rows in the last workgroup: one to four, ragged and full
    assert {(Lq - (Lq - 1) // 256 * 256 + 63) // 64 for _, Lq, _, _ in Q.QOUT_ASM_CASES} == {1, 2, 3, 4}
    for g in Q.QOUT_ASM_CASES[12:]:                       # the adjacent pairs: a seam inside a tile
        (s0, n0), (s1, _) = g[3]
        assert s1 == s0 + n0 and n0 % 64


@pytest.mark.parametrize("geom,fmt", ALL, ids=_ids)
def test_construction_conditions(geom, fmt):
    p = Q.Picked.get(geom, fmt)
    B, Lq, H = p.B, p.Lq, p.H
    print(f"{p}: worst |dot| {p.worst_dot:.0f}, lead {p.lead:.1f} binary orders")
    assert p.lead > 150 and p.worst_dot < 69
    first, last = p.start, p.end - 1
    assert ((p.pos >= first) & (p.pos <= last)).all()
    if Lq > 1:
        for b in range(B):
            for h in range(H):
                assert first in p.pos[b, h] and last in p.pos[b, h], (b, h)
                if Lq <= p.n:
                    assert len(set(p.pos[b, h])) == Lq                    # a permutation: no two rows of a head share a key
    else:
        assert first in p.pos and last in p.pos
    assert not np.array_equal(p.pos[0, 0], p.pos[-1, -1]) or (B * H == 1)
    # decoys: the slot below the range, the slot at its end and the rest of a ragged last tile, then every other outside slot
    tile_end = p.start + 64 * p.nt
    must = ([p.start - 1] if p.start else []) + list(range(p.end, tile_end + 1))
    assert must == p.near and set(p.near) <= set(p.outside) and len(p.outside) + p.n == p.Sk
    kv, vv = Q.bf16_val(p.k), Q.bf16_val(p.v)
    for (b, h, j), r in p.decoy_row.items():
        assert np.array_equal(kv[b, j, h], kv[b, p.pos[b, h, r], h]) and np.abs(vv[b, j, h]).min() >= 4096.0
    # ... and admitting one changes the bytes of the row it is aimed at (l = 2: the mean of the two V rows)
    b, h = B - 1, H - 1
    for j in p.near:
        r = p.decoy_row[(b, h, j)]
        x = np.zeros((1, H, 128), dtype=np.float32)
        x[0, h] = 0.5 * (vv[b, p.pos[b, h, r], h] + vv[b, j, h])
        H2 = H + (H & 1)
        full = np.zeros((1, H2 * 128), dtype=np.float32)
        full[0, :H * 128] = x.reshape(-1)
        codes, scales = QUANT[fmt](torch.from_numpy(full).to(torch.bfloat16))
        cols = head_code_bytes(fmt, h)
        row = b * Lq + r
        assert not (np.array_equal(np.asarray(codes).reshape(1, -1).view(np.uint8)[0, cols], p.codes[row, cols]) and
                    np.array_equal(np.asarray(scales).reshape(1, -1).view(np.uint8)[0, 4 * h:4 * h + 4], p.scales[row, 4 * h:4 * h + 4])), j


@pytest.mark.parametrize("geom,fmt", ALL, ids=_ids)
def test_expected_bytes_hold_the_edges(geom, fmt):
    p = Q.Picked.get(geom, fmt)
    B, Lq, H = p.B, p.Lq, p.H
    sc = p.scales.reshape(B, Lq, H, 4)
    cd = p.codes.reshape(B, Lq, -1)
    assert (sc == 0).any(), "no clamped exponent"
    zero_blocks = [(b, r, h, db) for b, r, h, db in np.argwhere(sc == 127) if not cd[b, r, block_bytes(fmt, h, db)].any()]
    assert zero_blocks, "no all-zero block under scale byte 127"
    assert len(np.unique(sc)) > (8 if B * Lq * H >= 64 else 3)                    # block maxima over several binades
    # edge blocks on rows of the first and of the last wave of the last workgroup, in both halves of each wave that has them
    zones = Q.edge_zones(Lq)
    q0 = (Lq - 1) // 256 * 256
    last_wave = (Lq - q0 - 1) // 64
    assert {w for w, _, _ in zones} == {0, last_wave}
    for w in (0, last_wave):
        assert {half for ww, half, _ in zones if ww == w} == ({0, 1} if Lq - q0 - 64 * w > 32 else {0})
    for w, half, rows in zones:
        assert all(q0 + 64 * w + 32 * half <= r < min(q0 + 64 * w + 32 * half + 32, Lq) for r in rows)
        if len(rows) == 4:                                                        # twelve edge slots: all ten (block, rotation) pairs
            for b in range(B):
                for h in range(H):
                    z = sc[b, rows, h]
                    assert (z == 127).any() and (z == 0).any(), (w, half, b, h)
    # the rotated blocks put a block maximum on the upper 32 lanes' channels (8 g4 + 4 .. 7) and the plain ones on the lower's
    x = np.abs(Q.bf16_val(p.rows_bits).reshape(B, Lq, H, 4, 32))
    am = x.argmax(-1)
    assert ((am % 8) >= 4).any() and ((am % 8) < 4).any()
    # distinct heads of a row have distinct code bytes
    per_head = np.stack([cd[:, :, head_code_bytes(fmt, h)] for h in range(H)], 2)          # [B, Lq, H, bytes]
    for h1 in range(H):
        for h2 in range(h1 + 1, H):
            assert (per_head[:, :, h1] != per_head[:, :, h2]).any(-1).all(), (h1, h2)


# ---- the generated text on the emulator ----------------------------------------------------------------------------------------
EMU_LQ = (1, 31, 33, 127, 255)                         # one workgroup, rows_valid <= 256
EMU = [(g, f) for g in Q.QOUT_ASM_CASES if g[1] in EMU_LQ for f in Q.FMTS]


def emu_case(text, geom, fmt, b=None, head=None):
    """One (batch element, head) of a geometry -- by default the last of each -- through the emulator: the whole sentinel-filled code
    and scale buffers against expected() of the picked V rows."""
    p = Q.Picked.get(geom, fmt)
    b = p.B - 1 if b is None else b
    head = p.H - 1 if head is None else head
    out_bits = p.rows_bits[b, :, head]
    assert np.array_equal(out_bits, p.v[b, p.pos[b, head], head])
    codes, scales = run(text, "lazy", p.q[b], p.k[b], p.v[b], p.Lq, p.n, p.H, head, p.start, fmt=fmt)
    wc, ws = expected(fmt, out_bits, p.H, head)
    # expected() quantises the head alone; the construction quantised whole rows: the head's bytes agree
    cols = head_code_bytes(fmt, head)
    rows = slice(b * p.Lq, (b + 1) * p.Lq)
    assert np.array_equal(wc[:p.Lq][:, cols], p.codes[rows][:, cols]) and np.array_equal(ws[:p.Lq, 4 * head:4 * head + 4],
                                                                                       p.scales[rows, 4 * head:4 * head + 4])
    assert (wc[p.Lq:] == SENT).all() and (ws[p.Lq:] == SENT).all() and wc.shape == (256, p.H * 16 * BITS[fmt])
    assert np.array_equal(scales, ws), (p, "scales", np.argwhere(scales != ws)[:8])
    assert np.array_equal(codes, wc), (p, "codes", np.argwhere(codes != wc)[:8])


@pytest.mark.parametrize("geom,fmt", EMU, ids=_ids)
def test_generated_text_writes_the_expected_bytes_on_the_emulator(texts, geom, fmt):
    assert sorted({g[1] for g, _ in EMU}) == list(EMU_LQ)
    emu_case(texts[fmt], geom, fmt)
