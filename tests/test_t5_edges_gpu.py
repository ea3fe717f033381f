"""The umT5 kernels (csrc/t5.hip) at their shape and stride edges, through the C ABI with explicit strides (ops.t5_attention always
passes ldqk = 2 H 64 and ldo = H 64).

ll_t5_attention runs the position and mask constructions of tests/vae_exact.py (T5Case): q = 0, so a score is the bias alone; one
large table entry per head turns query i into V[i + d] -- which pins bias_tab[key - query + L - 1] for every offset class -- and
every row without a key at that offset inside the mask into the mean of V over exactly seq_len keys (marker on key seq_len - 1,
-100 rows from seq_len on).  Bound: 2 bf16 ulp of the constructed expectation (P rounded once, the output once; the oracle's own
path measures <= 1.25 ulp on the host), a floor only at expected zeros; tests/test_vae_edges_host.py shows that one key more or fewer
or a bias offset moved by one moves an element by >= 64 x that bound.  q / k rows have ldqk > 2 H 64 with NaN padding, out rows
ldo > H 64 (ldo % 8 == 4 and == 0) in a NaN field with sentinel rows after L.

ll_t5_rmsnorm, ll_t5_gated_gelu and ll_gather_rows keep the bounds of tests/test_t5_gpu.py at the sizes that file never runs."""
import pytest
import torch

import vae_exact as E
from util import assert_bf16_close, bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = E.NAN16


def _run(fn, *args):
    from longlive_amd import _lib as L
    from longlive_amd import ops as O
    a = [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in args]
    L.check(getattr(L.load(), fn)(*a, O._stream()), fn)


def _nan_bf16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(bf)


def _untouched(t):
    return bool((t.contiguous().view(torch.int16) == NAN16).all())


@pytest.mark.parametrize("L,H,n,rot", E.T5_CASES, ids=str)
def test_t5_attention_position_and_mask_constructions(L, H, n, rot):
    case = E.T5Case(L, H, n, rot)
    C = H * 64
    exp = case.expected()
    bound = case.bound(exp).view(L, C).to(DEV)
    for ldqk, ldo in ((2 * C + 8, C + 4), (2 * C + 64, C + 8), (2 * C, C)):
        qk = _nan_bf16(L, ldqk)
        qk[:, :C] = 0.0
        qk[:, C:2 * C] = case.k().view(L, C).to(bf).to(DEV)
        vt = case.v().view(L, C).t().contiguous().to(bf).to(DEV)
        tab = case.table().to(bf).to(DEV)
        out = _nan_bf16(L + 3, ldo)
        _run("ll_t5_attention", qk, qk[:, C:], vt, tab, out, L, H, ldqk, ldo, n)
        torch.cuda.synchronize()
        assert _untouched(out[L:]) and _untouched(out[:L, C:]), f"wrote outside [L, H 64] (ldo {ldo})"
        got = out[:L, :C].double()
        assert torch.isfinite(got).all()
        err = (got - exp.view(L, C).to(DEV)).abs() / bound
        if err.max().item() > 1.0:
            i = int(err.argmax())
            r, c = i // C, i % C
            raise AssertionError(f"L={L} H={H} seq_len={n} ldqk={ldqk} ldo={ldo}: query {r} head {c // 64} (offset {case.d[c // 64]}) channel "
                                 f"{c % 64}: got {got[r, c].item()} want {exp.view(L, C)[r, c].item()} ({err.max().item():.1f} x the bound)")


@pytest.mark.parametrize("rows", [1, 70])
@pytest.mark.parametrize("C", [8, 520, 2048, 2056, 4096, 8192])
def test_t5_rmsnorm_at_the_column_loop_edges(rows, C):
    """One workgroup per row, 2048 columns per pass: C below one pass, 2048 | 2056 across it, 8192 = four passes; guard row after the output."""
    from oracle import ref_t5 as RT
    from longlive_amd import synth
    x = (synth.hash_normal(91, "ex", (rows, C)) * 2.0 + 0.1).to(bf)
    w = (synth.hash_normal(91, "ew", (C,)) * 0.1 + 1.0).to(bf)
    out = _nan_bf16(rows + 1, C)
    from ctypes import c_float
    _run("ll_t5_rmsnorm", x.to(DEV), w.to(DEV), out, rows, C, c_float(1e-6))
    torch.cuda.synchronize()
    assert _untouched(out[rows:])
    assert_bf16_close(out[:rows], RT.t5_layer_norm(x, w), 1, 0.99, f"t5_rmsnorm {rows}x{C}")


@pytest.mark.parametrize("M,F", [(1, 8), (37, 8), (1, 520), (3, 2056), (70, 24)])
def test_t5_gated_gelu_off_the_block(M, F):
    """F = 8 (one vector per row), M F / 8 not a multiple of the 256 threads of a block, M = 1; the bound and atol of test_t5_gated_gelu."""
    from oracle import ref_t5 as RT
    from longlive_amd import synth
    assert (M * F // 8) % 256 != 0
    h = (synth.hash_normal(91, "eh", (M, 2 * F)) * 1.5).to(bf)
    want = h[:, F:] * RT.gelu_py(h[:, :F])
    out = _nan_bf16(M + 1, F)
    _run("ll_t5_gated_gelu", h.to(DEV), out, M, F)
    torch.cuda.synchronize()
    assert _untouched(out[M:])
    assert_bf16_close(out[:M], want, 2, 0.98, f"t5_gated_gelu {M}x{F}", atol=2e-2)


@pytest.mark.parametrize("n", [1, 5, 7])
@pytest.mark.parametrize("C", [8, 512, 520, 4096])
def test_gather_rows_bit_exact_with_guard_rows(n, C):
    vocab = 37
    table = E._codes((vocab, C), C, -100, 100).to(bf)
    ids = torch.tensor([vocab - 1, 0, 7, 7, 36, 0, 19][:n], dtype=torch.long)
    out = _nan_bf16(n + 2, C)
    _run("ll_gather_rows", table.to(DEV), ids.to(DEV), out, n, C, vocab)
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    assert torch.equal(out[:n].cpu(), table[ids])
