"""Host proof of the MXFP8 attention edge suite (tests/mx_attn_exact.py; the GPU side is tests/test_mx_attn_edges_gpu.py).

For every exact-data case: the inputs quantise exactly; the magnitude span of every running l and O (rescaled carries included) stays
inside 24 bits, so every sum is exact in fp32 in any order -- the MFMA's internal order is not ours to assume; the restatement gives
the same bits in fp32 and in fp64 with the keys of every tile permuted; no expected element lies within 3 fp32 ulp of a bf16 rounding
tie, so the bf16 output has one bit pattern.  The restatement is held to an independent fp64 softmax over the dequantised shadows.
Every listed departure from the scheme moves the expected bf16 bits of at least one case -- but leaving adjacent ranges unmerged,
which must move none.  The plan counts, the refusals (nothing is launched: the library loads without a GPU) and the random-data
cases' own fp32 / fp64 distance are checked here too."""
import ctypes

import pytest
import torch

import mx_attn_exact as X
import mx_attn_ref as MA
from longlive_amd import _lib

KERNEL_BOUND = 3e-3          # tests/test_mx_attn_gpu.py's


@pytest.mark.parametrize("case", X.EXACT_CASES + X.QOUT_EVEN, ids=repr)
def test_case_is_exact_in_any_order(case):
    b = X.Built.get(case)
    # operands: the shadows and Q^ dequantise to the bf16 inputs
    S = case.S
    assert torch.equal(b.kd[:, :S], b.k.double()) and torch.equal(b.vd[:, :S], b.v.double())
    assert not b.kd[:, S:].any() and not b.vd[:, S:].any()
    qd = MA.mx_ref.dequantize(*MA.mx_ref.quantize(b.q.reshape(-1, 128))).reshape(b.q.shape)
    assert torch.equal(qd, b.q.double())
    span = X.span_report(b)
    assert span["l"] <= 24 and span["O"] <= 24, span
    assert torch.isfinite(b.want32).all()
    assert torch.equal(b.run(dtype=torch.float64), b.want32)
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        assert torch.equal(b.run(perm=g), b.want32) and torch.equal(b.run(dtype=torch.float64, perm=g), b.want32)
    assert X.tie_distance(b.want32).min().item() > 3


@pytest.mark.parametrize("case", X.EXACT_CASES + X.QOUT_EVEN, ids=repr)
def test_restatement_vs_independent_fp64_softmax(case):
    b = X.Built.get(case)
    out, bound = X.rounding_error_bound(b)
    over = (b.want32.double() - out).abs() - bound - 2.0 ** -22 * out.abs()      # + the two fp32 roundings of O x (1 / l)
    assert over.max().item() <= 0, (case, over.max().item())
    # and the bound is no blank cheque: on the boundary-marker data (integer levels: the bound is the two roundings alone) dropping
    # the last key of the first range leaves it somewhere
    mutant = X.run_mutant(b, "mask:hi0-") if case.levels is None and case.segs[0][1] - case.segs[0][0] > 1 else None
    if mutant is not None:
        assert ((mutant.double() - out).abs() > bound).any(), case


MUTATION_CASES = X.LAZY + X.TWO + X.ENDS + X.ZERO + [c for c in X.GEOMETRY if c.name in ("s1n33", "s31n65", "s96n64", "s33n129", "s127n1")]


def _moved(mut):
    return [c.name for c in MUTATION_CASES if not torch.equal(X.run_mutant(X.Built.get(c), mut).to(X.bf), X.Built.get(c).want)]


@pytest.mark.parametrize("mut", X.LOOP_MUTS + X.DATA_MUTS)
def test_mutation_moves_expected_bits(mut):
    moved = _moved(mut)
    print(f"{mut}: moves {len(moved)} of {len(MUTATION_CASES)} cases: {moved}")
    assert moved, mut


def test_lazy_constructions_catch_what_they_were_built_for():
    """The threshold and rounding mutations are caught by the lazy-max constructions themselves, the range-end shifts by every
    two-range case (an end on the edge of the range's tiles admits nothing when it moves outwards)."""
    lazy = {c.name for c in X.LAZY}
    for mut in ("nonlazy", "ge", "flush", "trunc", "l_unrounded", "no_l_rescale", "no_o_rescale"):
        assert lazy & set(_moved(mut)), mut
    assert "lazy_move9_stay8" in _moved("ge") and "lazy_move9_stay8" in _moved("nonlazy")
    assert "lazy_first_only" not in _moved("nonlazy")                       # its maximum never rises: the mutant is the scheme there
    for mut in X.MASK_MUTS:
        moved = set(_moved(mut))
        for c in X.TWO:
            if c.name == "two_adjacent":
                continue                                                    # one merged range: its seam is no range end
            g, end, d = int(mut[7]), mut[5:7], mut[8]
            lo, hi = c.segs[g]
            if (end == "lo" and d == "-" and lo % 32 == 0) or (end == "hi" and d == "+" and (hi - (lo & ~31)) % 64 == 0):
                continue                                                    # the admitted slot lies outside the range's tiles
            assert c.name in moved, (mut, c)


def test_unmerged_adjacent_ranges_give_the_same_bits():
    b = X.Built.get(next(c for c in X.TWO if c.name == "two_adjacent"))
    assert len(MA.tiles(b.case.segs, merge=False)) > len(MA.tiles(b.case.segs))      # the walk differs (the seam is not tile-aligned)
    assert torch.equal(X.run_mutant(b, "unmerged"), b.want32)


def test_lazy_reference_moves_where_the_constructions_say():
    """M per tile of row 0, from the restatement's own trace."""
    want = {"lazy_move9_stay8": [True, True, False], "lazy_rise_every_tile": [True, True, True],
            "lazy_first_only": [True, False, False, False], "lazy_last_only": [True, False, False, True], "lazy_from_32": [True, False]}
    for c in X.LAZY:
        moves, top = [], []
        X.Built.get(c).run(hook=lambda t: (moves.append(bool((t["Mn"] != t["M"])[0, 0, 0])), top.append(t["ph"][0, 0, 0].max().item())))
        assert moves == want[c.name], (c, moves)
        if c.name == "lazy_move9_stay8":
            assert top == [1.0, 1.0, 256.0]


@pytest.mark.parametrize("case", X.EXACT_CASES + X.QOUT_EVEN, ids=repr)
def test_plan_counts(case):
    from longlive_amd import ops
    nt, nr = case.plan_counts()
    p = ops.flash_attn_mx_plan(case.Lq, case.H, case.B, case.segs)
    wg = (case.Lq + 127) // 128 * case.H * case.B
    assert f"{wg} workgroups of 128 query rows, {nt} key tiles of 64 in {nr} range" in p, (p, nt, nr)


def test_geometry_lists_cover_what_they_claim():
    assert sorted({c.segs[0][0] % 64 for c in X.GEOMETRY}) == [0, 1, 31, 32, 33, 63]
    assert sorted({c.segs[0][1] - c.segs[0][0] for c in X.GEOMETRY}) == [1, 31, 32, 33, 63, 64, 65, 129]
    assert {c.S % 32 for c in X.ENDS if c.segs[0][1] == c.S} >= {0, 1, 31}
    for c in X.ENDS:
        if c.name.startswith("clamp"):
            assert (c.S32 // 32) % 2 == 1 and c.segs[0][0] // 32 == c.S32 // 32 - 1, c
    shared = next(c for c in X.TWO if c.name == "two_share_block")
    assert shared.segs[0][1] // 32 == shared.segs[1][0] // 32
    # the even-head list of the packed output formats: ROWS and BATCH again, a clamp case, H = 12, sweeps from 31 and 33
    assert all(c.H % 2 == 0 for c in X.QOUT_EVEN) and {c.H for c in X.QOUT_EVEN} == {2, 4, 12}
    assert (X.QOUT_ROWS.Lq, X.QOUT_ROWS.S, X.QOUT_ROWS.segs) == (X.ROWS.Lq, X.ROWS.S, X.ROWS.segs)
    assert (X.QOUT_BATCH.B, X.QOUT_BATCH.Lq, X.QOUT_BATCH.segs) == (X.BATCH.B, X.BATCH.Lq, X.BATCH.segs)
    assert X.QOUT_BATCH.segs[0][0] > X.QOUT_BATCH.segs[1][0]                  # two ranges in reverse order
    clamp = [c for c in X.QOUT_EVEN if "clamp" in c.name]
    assert clamp and all((c.S32 // 32) % 2 == 1 and c.segs[0][0] // 32 == c.S32 // 32 - 1 for c in clamp)
    assert {c.segs[0][0] for c in X.QOUT_EVEN if len(c.segs) == 1 and c.H == 2} >= {31, 33}
    assert any(c.H == 12 and c.Lq == 33 for c in X.QOUT_EVEN)


# ---- refusals: nothing is launched (no GPU here), the message names the argument --------------------------------------------------
def _mx(L, **kw):
    a = dict(B=1, Lq=64, H=3, hd=128, ldq=384, ldo=384, S=100, S32=128, s0=0, n0=50, s1=0, n1=0, scale=0.1)
    a.update(kw)
    return L.ll_flash_attn_mx(1, 1, 1, 1, 1, 1, a["B"], a["Lq"], a["H"], a["hd"], a["ldq"], a["ldo"], a["S"], a["S32"], a["s0"], a["n0"],
                              a["s1"], a["n1"], a["scale"], None)


@pytest.mark.parametrize("kw,needle", [
    (dict(s1=40, n1=30), "overlap"), (dict(s0=40, n0=30, s1=0, n1=41), "overlap"), (dict(s1=0, n1=50), "overlap"),
    (dict(s0=10, n0=40, s1=20, n1=5), "overlap"),
    (dict(scale=0.0), "scale="), (dict(scale=-0.1), "scale="), (dict(scale=float("nan")), "scale="), (dict(scale=float("inf")), "scale="),
    (dict(S32=96), "S32=96"), (dict(S32=160), "S32=160"), (dict(n0=101), "first key range"), (dict(s1=90, n1=11), "second key range"),
    (dict(hd=64), "head_dim=64"), (dict(ldq=388), "row strides"), (dict(ldo=386), "row strides"), (dict(ldq=376), "row strides"),
    (dict(ldo=380), "row strides"),
])
def test_flash_attn_mx_refusals(kw, needle):
    L = _lib.load()
    assert _mx(L, **kw) == -1
    assert needle in L.ll_last_error().decode()


def test_ranges_that_only_touch_are_accepted_arguments():
    """[0, 50) + [50, 100) and a second range before the first pass the checks (B = 0: accepted, nothing to launch)."""
    L = _lib.load()
    assert _mx(L, B=0, s1=50, n1=50) == 0 and _mx(L, B=0, s0=50, n0=50, s1=0, n1=50) == 0 and _mx(L, B=0, s0=60, n0=40, s1=3, n1=20) == 0


def test_flash_attn_refuses_overlapping_ranges():
    L = _lib.load()
    for s0, n0, s1, n1 in ((0, 50, 40, 30), (40, 30, 0, 41), (0, 50, 0, 50)):
        assert L.ll_flash_attn(1, 1, 1, 1, 1, 64, 3, 384, 384, 384, 384 * 100, s0, n0, s1, n1, 0.1, None) == -1
        assert "overlap" in L.ll_last_error().decode()
    assert L.ll_flash_attn(1, 1, 1, 1, 0, 64, 3, 384, 384, 384, 384 * 100, 50, 50, 0, 50, 0.1, None) == 0


def test_no_caller_passes_overlapping_ranges():
    """kv_cache.plan_update's two ranges are the sink [0, sink) and a window that starts at or after it."""
    from longlive_amd.kv_cache import plan_update
    for fs, sink in ((13, 1), (40, 2), (7, 0)):
        G = E = 0
        for f in range(14):
            plan = plan_update(f * fs, fs, G, E, 4 * fs, sink * fs, 4, 4 * fs)
            G, E = plan.G_new, plan.E_new
            segs = sorted(plan.segments)
            assert 1 <= len(segs) <= 2 and all(a[1] <= b[0] for a, b in zip(segs, segs[1:])), plan.segments


# ---- the random-data cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.RANDOM))
def test_random_cases_restatement_is_stable(name):
    """The restatement's own fp32-vs-fp64 distance stays below a third of the kernel bound at these shapes."""
    B, Lq, H, S, segs = X.RANDOM[name]
    q, k, v = X.random_data(B, Lq, H, S)
    a = MA.mx_attention_cache(q, k, v, segs).to(X.bf).double()
    b = MA.mx_attention_cache(q, k, v, segs, dtype=torch.float64).to(X.bf).double()
    r = ((a - b).norm() / b.norm()).item()
    print(f"{name}: restatement fp32 vs fp64 (bf16 outputs) relL2 {r:.2e}")
    assert r < KERNEL_BOUND / 3, r
