"""The constructions of tests/test_bf16_edges_gpu.py (tests/bf16_exact.py), proved on the host: the GEMM data sets are exact (the
constructor asserts the bounds on the sums), and for every attention geometry of the GPU module the oracle's own bf16 path stays
inside the tolerance the GPU tests use while every single-key mutation of the key set -- one in-range boundary key dropped, one
out-of-range slot admitted -- moves at least one output element by >= 8 x that tolerance.  Mutations are applied to the host
reference only.

Measured here (every geometry with its own head count, both phases; sums and mutations on head 0, the lead on every head): the fp64
attention of the construction is within 1.5e-10 of the expected values (V[pi(r)] on gather rows, the mean on uniform rows), the
target key's smallest lead is 32.6 binary orders (18720 keys x 12 heads; 37.7 at 1437 keys x 12 heads), and the oracle's bf16 path
(oracle.ref_ops.attention) is at most 0.51 bf16 ulp away (0 on gather rows), so the bound is
the 2 ulp of the number format."""
import pytest
import torch

import bf16_exact as E
from oracle import ref_ops as R

HOST_ROWS = 1000        # rows of the production shapes checked here (they aim at every target of the 18720-key range)


def _host_case(B, Lq, H, ranges, **kw):
    """The geometry with its own head count (the sign codes depend on it: the data checked here is the data the GPU runs), batch
    element 0 (element b is the same V rolled by b channels) and at most HOST_ROWS rows (rows are independent of one another)."""
    return E.AttnCase(1, min(Lq, HOST_ROWS), H, ranges, **kw)


def _check_geometry(case, qnorm=False):
    stats = {"exact": 0.0, "lead": float("inf"), "oracle_ulp": 0.0}
    worst = {}                                     # mutation -> the largest |moved| / bound over both phases
    for phase in (0, 1):
        q, k, v, exp = case.build(phase)
        if qnorm:
            _, q = case.q_raw_and_ssq(q)
        uni, tg = case.row_plan(phase)
        q0, k0, v0, exp0 = q[0, :, 0], k[0, :, 0], v[0, :, 0], exp[0, :, 0]
        for t in (q0, k0, v0):
            assert torch.equal(t.to(E.bf).double(), t)                       # bf16-exact inputs
        bound = E.attn_bound(exp0, case.nkeys)
        # (a) the reference: fp64 equals the construction's expected values, the oracle's bf16 path is inside the bound
        inr = torch.tensor(case.inr)
        qq, kk, vv = q0.view(1, -1, 1, 128), k0[inr].view(1, -1, 1, 128), v0[inr].view(1, -1, 1, 128)
        exact = R.attention_exact(qq, kk, vv)[0, :, 0]
        stats["exact"] = max(stats["exact"], (exact - exp0).abs().max().item())
        assert ((exact - exp0).abs() <= bound / 64).all()
        oracle = R.attention(qq, kk, vv)[0, :, 0].double()
        assert ((oracle - exp0).abs() <= bound).all(), ((oracle - exp0).abs() / bound).max()
        nz = exp0 != 0
        stats["oracle_ulp"] = max(stats["oracle_ulp"], ((oracle - exp0).abs()[nz] / E.ulp_bf16(exp0)[nz]).max().item())
        for h in range(case.H if (~uni).any() else 0):                       # every head's lead
            stats["lead"] = min(stats["lead"], E.attn_lead(q[0, ~uni, h], k[0, :, h], case.inr).min().item())
        # (b) single-key mutations, on the rows they concern: the gather rows aimed at the key (or at the key whose code the admitted
        # slot carries) and one uniform row (all uniform rows are the same row)
        targeted = set(tg[~uni].tolist())
        muts = [("drop", j) for j in dict.fromkeys(case.range_bounds + [t for t in case.targets if t in targeted])]
        muts += [("admit", o) for o in case.outside]
        urow = uni.nonzero()[:1].flatten().tolist()
        for kind, j in muts:
            aim = j if kind == "drop" else case.poison_target[j]
            rows = ((~uni) & (tg == aim)).nonzero().flatten().tolist()[:2] + urow
            slots = [s for s in case.inr if s != j] if kind == "drop" else case.inr + [j]
            moved = 0.0
            if rows and slots:
                r = torch.tensor(rows)
                moved = ((E.attn_host(q0[r], k0, v0, slots) - exp0[r]).abs() / bound[r]).max().item()
            elif rows:                     # the only key dropped: no output at all
                moved = float("inf")
            worst[(kind, j)] = max(worst.get((kind, j), 0.0), moved)
    assert stats["lead"] >= E.LEAD_MIN, stats
    weak = {m: w for m, w in worst.items() if w < 8}
    assert not weak, f"mutations the construction would not see: {weak}"
    return stats


@pytest.mark.parametrize("geom", E.ALL_SMALL_CASES + E.PROD_CASES, ids=lambda g: f"B{g[0]}-Lq{g[1]}-H{g[2]}-{g[3]}")
def test_attention_constructions_are_exact_and_see_one_key(geom):
    st = _check_geometry(_host_case(*geom))
    print(geom, st)
    assert st["exact"] < 2e-9 and st["oracle_ulp"] <= E.ATTN_BOUND_ULP


@pytest.mark.parametrize("geom", E.QNORM_CASES, ids=lambda g: f"B{g[0]}-Lq{g[1]}-H{g[2]}-{g[3]}")
def test_qnorm_gather_is_exact_and_sees_one_key(geom):
    """The same through WanRMSNorm with a unit weight: the raw q of amplitude 2 normalises to the +-1 codes exactly, the keys carry
    amplitude 4, so the scores are the plain construction's."""
    case = _host_case(*geom, a_k=4.0)
    q = case.build(1)[0]
    ssq, qn = case.q_raw_and_ssq(q)
    uni, _ = case.row_plan(1)
    assert torch.equal(qn[0, ~uni].abs(), torch.ones_like(qn[0, ~uni])) and (qn[0, uni] == 0).all()
    assert torch.equal(ssq[0, ~uni], torch.full_like(ssq[0, ~uni], 512.0))
    st = _check_geometry(case, qnorm=True)
    print(geom, st)
    assert st["exact"] < 2e-9


def test_every_tile_seam_is_a_target_somewhere():
    """Small Lq cannot aim at every seam of a long range (range boundaries come first in the target order); for every kernel's case
    list at least one multi-tile geometry has enough gather rows to aim at every target, in both phases."""
    for cases in (E.PIPE0_CASES, E.PIPE1_CASES, E.ASM_CASES, E.TWO_RANGE_CASES, E.PROD_CASES, E.QNORM_CASES):
        full = [g for g in cases if E.AttnCase(*g).nkeys > 2 * E.KT and (g[1] * 3) // 4 - 1 >= len(E.AttnCase(*g).targets)]
        assert full, cases


@pytest.mark.parametrize("M,N,K,unit", [(300, 384, 256, False), (65, 1536, 8960, False), (1100, 136, 64, False), (300, 2048, 256, True),
                                        (300, 448, 320, "o1"), (65, 224, 8960, "o1"), (300, 8, 64, "o1")])
def test_gemm_data_is_exact(M, N, K, unit):
    """The constructor's own assertions are the proof (operands exact in bf16, |sum of codes| <= 16 K < 2^24, acc + bias on a 2^-6 grid
    below 2^18); here: they hold at both ends of K, fp32 accumulation in two different orders gives the fp64 sums, and the expected
    output is the fp64 result rounded once."""
    d = E.GemmData(M, N, K, 3, unit is True, o1=unit == "o1")
    x, w = d.x.float(), d.w.float()
    fwd = x @ w.t()
    half = x[:, :K // 2] @ w[:, :K // 2].t()
    split = (x[:, K // 2:].flip(1) @ w[:, K // 2:].flip(1).t()) + half
    assert torch.equal(fwd.double(), d.acc) and torch.equal(split.double(), d.acc)
    assert torch.equal((fwd + d.bias.float()).to(E.bf), d.want)
    assert d.want.float().abs().max() > 0
    if unit is True:
        s = d.ssq(M)
        assert torch.equal(s.double(), s.double().round()) and s.max() < 2 ** 24


def test_gelu_data_keeps_torch_reference_well_conditioned():
    """The O(1) data set of the GELU cases: torch's bf16 tanh-GELU agrees with the fp64 value (x sigmoid(2u), no cancellation) on
    >= 99 % of its outputs there, against ~95 % on the wide scales of the default set (the tail -9 < x < -3)."""
    import math

    def frac(d):
        x = d.want.double()
        u = math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)
        return (torch.nn.functional.gelu(d.want, approximate="tanh") == (x * torch.sigmoid(2 * u)).to(E.bf)).float().mean().item()
    assert frac(E.GemmData(300, 448, 320, 5, o1=True)) >= 0.99
    assert frac(E.GemmData(300, 448, 320, 5)) < 0.97
