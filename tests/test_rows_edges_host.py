"""The constructions and host references of tests/test_rows_edges_gpu.py (tests/rows_exact.py), proved on the host.

Data: the exact rows have the properties claimed -- fp32 running sums of x and of the centred squares in two opposite orders and in
the kernels' lane order all equal the fp64 sums, the mean is exactly m, every stated partial-sum bound is below 2^24 -- and torch's
CPU fp32 divide / sqrt / reciprocal are the correctly rounded single operations the chains assume (each equals the fp64 operation
rounded once: 53 >= 2 x 24 + 2 bits make that double rounding innocuous).  The RoPE hash tables hold pairwise distinct entries.

Oracle: on generic hash-normal data the chains agree with oracle/ref_ops.py (ln_modulate, layer_norm, rms_norm, causal_rope_apply) to
the project's bound of 1 ulp with 99 % exact -- they restate the reference's rounding points, not the kernel's -- and on the exact
rows the same comparison is (almost) bit-exact; the measured shares are next to the assertions.

Mutations (applied to the references only): a dropped or added rounding point, C rounded up to whole chunks in the statistics, shift
and scale exchanged, the frame of row + 1, the RoPE handover moved by one, the pair index without the modulo, the write window one
slot further on, the argmin tie resolved upward -- each changes the expected bits of the case list written for it."""
import math

import pytest
import torch

import rows_exact as E
from oracle import ref_ops as R
from util import assert_bf16_close, bf16_ulp_distance

bf, f32 = E.bf, E.f32


def _same(a, b):
    return torch.equal(E.bits(a), E.bits(b))


# ---- data properties --------------------------------------------------------------------------------------------------------------------
def _lane_order(C):
    """Column order in which one lane adds its elements, lanes side by side: [64, n] column indices padded with -1 (chunks l, l + 64, ..)."""
    cols = torch.full((64, 4 * 8), -1, dtype=torch.int64)
    for lane in range(64):
        k = 0
        for i in range(4):
            for j in range(8):
                c = (lane + 64 * i) * 8 + j
                if c < C:
                    cols[lane, k] = c
                k += 1
    return cols


@pytest.mark.parametrize("C", E.WIDTHS)
def test_exact_rows_sum_exactly_in_any_order(C):
    x, m = E.exact_rows(42, C, seed=C)
    xd = x.double()
    assert torch.equal(xd.sum(-1), m * C) and torch.equal(E.op32(torch.div, xd.sum(-1).to(f32), float(C)).double(), m)       # the mean is exactly m
    d = xd - m.view(-1, 1)
    assert torch.equal(d * 4, (d * 4).round()) and float(d.abs().max()) <= 1.0
    assert not x[1].any() and not x[3, :E.last_chunk_start(C)].any() and x[3, E.last_chunk_start(C):].any()
    for t in (x.to(f32), (d * d).to(f32)):
        want = t.double().sum(-1)
        fwd, rev = torch.cumsum(t, -1), torch.cumsum(t.flip(-1), -1)                 # fp32 running sums, two opposite orders
        assert torch.equal(fwd.double(), torch.cumsum(t.double(), -1)) and torch.equal(rev.double(), torch.cumsum(t.double().flip(-1), -1))
        assert torch.equal(fwd[:, -1].double(), want) and torch.equal(rev[:, -1].double(), want)
        # the kernels' order: per lane over its chunks, then the butterfly over the lanes
        cols = _lane_order(C)
        tl = torch.cat([t, torch.zeros(t.shape[0], 1)], -1)[:, cols]                  # [rows, 64, 32], -1 -> the appended zero
        lane = torch.cumsum(tl, -1)[..., -1]
        for o in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[:, torch.arange(64) ^ o]
        assert torch.equal(lane[:, 0].double(), want)
    # rows of mean 0 (RMSNorm, q/k norm): the sum of x^2 is exact
    x0, _ = E.exact_rows(42, C, seed=C + 1, means=0.0)
    sq = (x0.to(f32) * x0.to(f32))
    assert torch.equal(torch.cumsum(sq, -1)[:, -1].double(), x0.double().pow(2).sum(-1))


def test_partial_sum_bounds_are_below_2_24():
    assert 12 * max(E.WIDTHS) < 2 ** 24 and 16 * max(E.WIDTHS) < 2 ** 24
    assert all(v < 2 ** 24 for v in E.LINEAR_CODE_BOUND.values()) and all(v < 2 ** 24 for v in E.LINEAR_ACT_IN_BOUND.values())
    for K in E.LINEAR_K:
        E.LinearData(8, 258, K)                      # the constructors assert the bound on the data itself
    for K in E.LINEAR_ACT_IN_K:
        E.LinearActInData(8, 258, K)


def test_single_fp32_operations_are_correctly_rounded_on_the_host():
    """rows_exact.op32 against numpy's float32 operations (IEEE single operations of the host's scalar / SSE units)."""
    import numpy as np
    v = (E.hnorm((4096,), 3).double().abs() * 37.0 + 2.0 ** -12).to(f32)
    vn = v.numpy()
    eps = np.float32(E.EPS)
    for C in E.WIDTHS:
        q = E.op32(torch.div, v, float(C))
        assert np.array_equal(q.numpy(), vn / np.float32(C))
        a = E.op32(torch.add, q, E.EPS)
        assert np.array_equal(a.numpy(), q.numpy() + eps)
        s = E.op32(torch.sqrt, a)
        assert np.array_equal(s.numpy(), np.sqrt(a.numpy()))
        r = E.op32(torch.reciprocal, s)
        assert np.array_equal(r.numpy(), np.float32(1.0) / s.numpy())
        assert torch.equal(E.inv_sqrt(v, C), r)
    assert float(E.inv_sqrt(torch.zeros(1), 8)) == float(np.float32(1.0) / np.sqrt(eps))      # the all-zero row: rstd = 1 / sqrt(eps)


@pytest.mark.parametrize("C,D", E.QK_SHAPES)
def test_rope_hash_tables_are_pairwise_distinct(C, D):
    for sf in E.QK_START_FRAMES:
        rf, rhw = E.rope_hash_tables(sf + E.QK_F, D, E.QK_FL)
        allv = torch.cat([rf.flatten(), rhw.flatten()])
        assert allv.unique().numel() == allv.numel() and float(allv.abs().max()) <= 1.0
        assert rf.shape == (sf + E.QK_F, E.rope_nf(D), 2) and rhw.shape == (E.QK_FL, D // 2 - E.rope_nf(D), 2)
    assert [E.rope_nf(d) for d in (128, 64, 40, 8)] == [22, 12, 8, 2]


def test_model_tables_are_the_references_angles():
    for D in (128, 64, 40, 8):
        fr = R.make_freqs(D)
        nf = E.rope_nf(D)
        rf, rhw = E.rope_model_tables(1024, D, 3, 5)
        assert torch.equal(rf[..., 0], fr[:, :nf].real.to(f32)) and torch.equal(rf[..., 1], fr[:, :nf].imag.to(f32))
        c3 = (D // 2) // 3
        assert torch.equal(rhw[7, :c3, 0], fr[1, nf:nf + c3].real.to(f32)) and torch.equal(rhw[7, c3:, 1], fr[2, nf + c3:].imag.to(f32))   # token 7 = (h 1, w 2)


# ---- oracle agreement -------------------------------------------------------------------------------------------------------------------
def _mod_inputs(B, F, C, seed):
    e = E.hnorm((B, F, 6, C), seed, 0.5)
    mod = E.hnorm((6, C), seed + 1, 1 / math.sqrt(C))
    return e, mod


def _exact_share(a, b):
    return float((bf16_ulp_distance(a, b) == 0).float().mean())


# Measured on the exact rows (42 rows, every width, both index pairs; the smallest share of bit-identical elements over the widths):
# ln_modulate 0.99994, layer_norm 0.99991 (F.layer_norm forms its statistics in another way; single ulps, and larger ulp distances
# only where the output cancels to near zero, which the project's bound leaves to its absolute floor), rms_norm 1.0 (bit-exact at
# every width), q/k norm + RoPE on the model's tables 0.99998 (1 ulp: fp32 tables against the fp64 complex product).
EXACT_ROWS_MIN_SHARE = 0.999


@pytest.mark.parametrize("C", E.WIDTHS)
def test_row_chains_agree_with_the_oracle(C):
    B, F, fl = 2, 3, 7
    e, mod = _mod_inputs(B, F, C, C)
    ec = (mod.view(1, 1, 6, C) + e).chunk(6, dim=2)                                   # causal_model.py:440
    w, b = E.hnorm((C,), C + 2, 0.1, 1.0), E.hnorm((C,), C + 3, 0.1)
    generic = (E.hnorm((B, F * fl, C), C + 4, 1.7, 0.3), 0.99)
    exact = (E.exact_rows(B * F * fl, C, seed=C)[0].view(B, F * fl, C), EXACT_ROWS_MIN_SHARE)
    for x, share in (generic, exact):
        for sh, sc in E.MOD_PAIRS:
            want = R.ln_modulate(x, ec[sc], ec[sh], F, E.EPS).reshape(-1, C)
            assert_bf16_close(E.ln_modulate_host(x, e, mod, sh, sc, F), want, 1, share, f"ln_modulate {sh},{sc}")
            tab = E.modulation_table_f32_host(e.view(B * F, 6, C), mod.view(1, 6, C), 0b010010)[0]
            assert _same(E.ln_modulate_tab_host(x, tab, sh, sc, F), E.ln_modulate_host(x, e, mod, sh, sc, F))
            pre = E.modulation_table_host(e.view(B * F, 6, C), mod.view(1, 6, C))[0]
            assert _same(E.ln_modulate_host(x, pre, None, sh, sc, F), E.ln_modulate_host(x, e, mod, sh, sc, F))
        x2 = x.reshape(-1, C)
        assert_bf16_close(E.layernorm_affine_host(x2, w, b), R.layer_norm(x2, E.EPS, w, b), 1, share, "layer_norm")
    for x, share in ((generic[0].reshape(-1, C), 0.99), (E.exact_rows(42, C, seed=C + 1, means=0.0)[0], EXACT_ROWS_MIN_SHARE)):
        assert_bf16_close(E.rmsnorm_host(x, w), R.rms_norm(x, w, E.EPS), 1, share, "rms_norm")


@pytest.mark.parametrize("C,D", E.QK_SHAPES)
def test_qk_chain_agrees_with_the_oracle(C, D):
    """Model tables against causal_rope_apply (fp64 complex product of the fp64 table, rounded once) of the oracle's rms_norm."""
    d = E.QKData(C, D)
    B, L, H = d.B, d.L, C // D
    freqs = R.make_freqs(D)
    gen = E.hnorm((B * L, C), 5, 1.3)
    for sf in E.QK_START_FRAMES:
        rf, rhw = d.tables("model", sf)
        for x, w, share in ((gen, d.wq, 0.99), (d.q, d.wq, EXACT_ROWS_MIN_SHARE), (d.k, d.wk, EXACT_ROWS_MIN_SHARE)):
            want = R.causal_rope_apply(R.rms_norm(x, w, E.EPS).view(B, L, H, D), (d.F, 3, 5), freqs, sf).reshape(B * L, C)
            got = E.qk_rope_host(x, w, rf, rhw, L, d.fl, sf, D)
            assert_bf16_close(got, want, 1, share, f"rope {C},{D} start {sf}")


# ---- mutations --------------------------------------------------------------------------------------------------------------------------
def _row_cases():
    for C in E.WIDTHS:
        for B, F, fl in E.ROW_GEOS:
            yield C, B, F, fl


def test_row_mutations_change_the_expected_bits():
    hit = {k: 0 for k in ("no_round_y", "cpad", "swap", "frame+1", "tab swap", "tab frame+1", "tab cpad", "affine round_y", "affine cpad",
                          "rms no_round_y")}
    ragged = 0
    for C, B, F, fl in _row_cases():
        x = E.exact_rows(B * F * fl, C, seed=C + B)[0].view(B, F * fl, C)
        e, mod = _mod_inputs(B, F, C, C)
        tab = E.modulation_table_f32_host(e.view(B * F, 6, C), mod.view(1, 6, C), 0b010010)[0]
        w, b = E.hnorm((C,), C + 2, 0.1, 1.0), E.hnorm((C,), C + 3, 0.1)
        for sh, sc in E.MOD_PAIRS:
            base, tbase = E.ln_modulate_host(x, e, mod, sh, sc, F), E.ln_modulate_tab_host(x, tab, sh, sc, F)
            for mu in ("no_round_y", "cpad", "swap", "frame+1"):
                changed = not _same(E.ln_modulate_host(x, e, mod, sh, sc, F, mut=(mu,)), base)
                hit[mu] += changed
                if mu == "swap" or (mu == "frame+1" and F > 1) or (mu == "cpad" and C % 512):
                    assert changed, (mu, C, B, F, fl)                                  # every case that can see the fault does
                if mu != "no_round_y":
                    tchanged = not _same(E.ln_modulate_tab_host(x, tab, sh, sc, F, mut=(mu,)), tbase)
                    hit["tab " + mu] += tchanged
                    assert tchanged == changed or mu == "cpad", (mu, C)
        x2 = x.reshape(-1, C)
        abase = E.layernorm_affine_host(x2, w, b)
        hit["affine round_y"] += not _same(E.layernorm_affine_host(x2, w, b, mut=("round_y",)), abase)
        hit["affine cpad"] += not _same(E.layernorm_affine_host(x2, w, b, mut=("cpad",)), abase)
        x0 = E.exact_rows(B * F * fl, C, seed=C + 1, means=0.0)[0]
        hit["rms no_round_y"] += not _same(E.rmsnorm_host(x0, w, mut=("no_round_y",)), E.rmsnorm_host(x0, w))
        ragged += bool(C % 512)
    assert all(v > 0 for v in hit.values()), hit
    assert hit["cpad"] >= 2 * ragged and hit["affine cpad"] >= ragged


@pytest.mark.parametrize("C,D", E.QK_SHAPES)
def test_qk_mutations_change_the_expected_bits(C, D):
    d = E.QKData(C, D)
    for sf in E.QK_START_FRAMES:
        q0, k0 = d.expected("hash", sf)
        for mu in ("frame+1", "nf+1", "nf-1", "no_mod", "no_round_y"):
            q1, k1 = d.expected("hash", sf, mut=(mu,))
            if mu == "no_mod" and C == D:
                assert _same(q1, q0)                                                   # one head: nothing to reduce
                continue
            assert not _same(q1, q0) and not _same(k1, k0), (mu, C, D, sf)
    # the handover pair itself: pairs nf - 1 and nf of head 0 and of the last head change under the two nf mutations
    nf, half = E.rope_nf(D), D // 2
    q0 = d.expected("hash", 0)[0]
    for mu, p in (("nf+1", nf), ("nf-1", nf - 1)):
        q1 = d.expected("hash", 0, mut=(mu,))[0]
        for head in (0, C // D - 1):
            col = head * D + 2 * p
            assert not _same(q1[:, col:col + 2], q0[:, col:col + 2])
    # the write window one slot further on
    _, k = d.expected("hash", 0)
    for S, ws, ro, wl in E.QK_WINDOWS:
        cache = torch.full((d.B, S + 1, C), float("nan"), dtype=bf)
        a, b = E.kv_insert_host(cache, k, S, ws, ro, wl), E.kv_insert_host(cache, k, S, ws, ro, wl, mut=("window+1",))
        assert _same(a, b) == (wl == 0)


def test_sigma_lookup_reference_and_its_tie_mutation():
    tabs = E.sigma_tables()
    ties = 0
    for name, (ts, sg) in tabs.items():
        q = E.sigma_queries(ts)
        want = E.sigma_lookup_host(q, ts, sg)
        n = ts.numel()
        if name != "repeat":
            assert torch.equal(want[:n], sg)                                          # a table value finds its own entry
        else:
            assert want[21] == sg[20] and want[20] == sg[20]                           # the repeated timestep: the lower index
        assert want[-3] == sg[0] and want[-2] == sg[0] and want[-1] == sg[0]           # +-inf and NaN: torch.argmin's index 0
        assert want[n + n - 1] == sg[ts.argmin()] and want[n + n + 1] == sg[ts.argmax()]        # beyond the two ends
        up = E.sigma_lookup_host(q, ts, sg, mut=("tie_up",))
        if name != "real":
            assert not torch.equal(up, want), name
            mid = want[n:2 * n - 1]
            if name != "repeat":
                assert torch.equal(mid, sg[:-1])                                      # an exact midpoint: the lower index
        ties += int((up != want).sum())
    assert ties > 0
    assert int(torch.argmin(torch.full((1, 7), float("nan"), dtype=torch.float64), 1)) == 0
    assert int(torch.argmin(torch.full((1, 7), float("inf"), dtype=torch.float64), 1)) == 0


# ---- ll_linear_small --------------------------------------------------------------------------------------------------------------------
def test_act_in_grid_is_determined_and_sums_exactly():
    x, s = E.linear_act_in_values()
    assert len(x) >= 33 - E.SILU_MAX_DROPPED
    # torch's own fp32 SiLU rounded to bf16 gives the determined value on every kept grid point
    assert torch.equal(torch.nn.functional.silu(x.to(f32)).to(bf).double(), s)
    for K in E.LINEAR_ACT_IN_K:
        d = E.LinearActInData(8, 258, K)
        xs = torch.nn.functional.silu(d.x.to(f32)).to(bf).to(f32)
        assert torch.equal(torch.cumsum(xs[:, None, :] * d.w.to(f32)[None], -1)[..., -1].double(), d.acc)     # fp32 running sum = fp64


# torch's fp32 SiLU rounded to bf16 against fp64 SiLU of the same exact pre-activations rounded once, over every (M, N) of a K (3180
# outputs each): bit-exact on all of them at every K (share 1.0, 0 ulp).  The kernel's share is held against this in the GPU module.
TORCH_SILU_SHARE = {8: 1.0, 504: 1.0, 512: 1.0, 520: 1.0, 1536: 1.0}


def torch_silu_share(K):
    """(share of bit-exact outputs, largest ulp distance) of torch's fp32 SiLU over every (M, N) of the GPU test's list at this K."""
    got, want = [], []
    for M in E.LINEAR_M:
        for N in E.LINEAR_N:
            d = E.LinearData(M, N, K)
            got.append(torch.nn.functional.silu(d.pre.to(f32)).to(bf).flatten())
            want.append(d.silu64().to(bf).flatten())
    dist = bf16_ulp_distance(torch.cat(got), torch.cat(want))
    return float((dist == 0).float().mean()), int(dist.max())


@pytest.mark.parametrize("K", E.LINEAR_K)
def test_linear_data_is_exact_and_torch_silu_share(K):
    for M in E.LINEAR_M:
        for N in E.LINEAR_N:
            d = E.LinearData(M, N, K)
            p = d.x.to(f32)[:, None, :] * d.w.to(f32)[None]
            assert torch.equal(torch.cumsum(p, -1)[..., -1].double(), d.acc) and torch.equal(torch.cumsum(p.flip(-1), -1)[..., -1].double(), d.acc)
            assert float(d.pre.double().abs().max()) < 16 and d.pre.double().std() > 0.05 if M * N > 8 else True
    share, worst = torch_silu_share(K)
    print(f"torch fp32 SiLU share at K = {K}: {share:.4f}, worst {worst} ulp")
    assert worst <= 1 and abs(share - TORCH_SILU_SHARE[K]) < 5e-4
