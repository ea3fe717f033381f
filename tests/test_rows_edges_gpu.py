"""The row, cache and latent kernels (csrc/elementwise.hip) and ll_linear_small (csrc/gemm.hip) at their shape edges, through the C ABI
with explicit pointers and strides (the ops.* wrappers allocate exact-size contiguous outputs and cannot place guards).

Row kernels run on the exact rows of tests/rows_exact.py: both wave reductions are exact in any order and every other step is one
IEEE fp32 operation, so the output has ONE correct bit pattern -- the reference's rounding chain evaluated on the host -- and is
compared on the bf16 bits.  Every output lies in a field of NAN16 with three sentinel rows after the last row (ll_rmsnorm: ldo = C + 8
as well), every input is followed by NaN rows, the RoPE tables end in NaN rows directly after the last row a case may read, and the
KV cache is a NaN field whose every slot outside the write window must keep its bits.

Which kernel instance a case launches (DISPATCH_NCH: NCH = ceil(C / 512), FULL = C % 512 == 0):

    C      8   256   512   520   768  1024  1280  1536  1792  2040  2048
    NCH    1     1     1     2     2     2     3     3     4     4     4
    FULL   -     -   yes     -     -   yes     -   yes     -     -   yes      (520: a ragged chunk of one lane, 2040: of 63 lanes)

  test_ln_modulate[C]           ln_modulate_kernel<NCH, FULL, PRE 0 and 1, EmitBf16Q8>      every column
  test_ln_modulate_tab[C]       ln_modulate_tab_kernel<NCH, FULL, EmitBf16Q8>               every column
  test_layernorm_affine[C]      layernorm_affine_kernel<NCH, FULL, EmitBf16Q8>              every column
  test_rmsnorm[C]               rmsnorm_kernel<NCH, FULL>                                   every column
  test_qk_norm_rope_kv_store    qk_norm_rope_kv_kernel<1>: C 256 and 8 (one lane);  <2>: C 1024 (whole), 768 and 520 (ragged);
                                <3>: C 1536;  <4>: C 2048
  (ll_rmsnorm in place -- out == x -- is not run: no caller in model.py uses it, and the kernel declares both pointers __restrict__.)

The cache and latent kernels are bit-exact by construction (copies, permutations, fp64 / separately rounded fp32 expressions);
ll_sinusoid keeps the project's bound (1 ulp, 98 % exact per half row) and ll_linear_small's act_out = 1 the one of
rows_exact.SILU_SHARE_SLACK; nothing else in this module has a tolerance."""
import math

import pytest
import torch

import rows_exact as E
from util import assert_bf16_close, bf, bf16_ulp_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = E.NAN16
NAN32 = 0x7FC12345                 # the fp32 sentinel pattern
f32 = torch.float32
INVALID = -1                       # LL_ERR_INVALID_ARG


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def _lib():
    from longlive_amd import _lib as L
    return L, L.load()


def _call(fn, *args):
    from longlive_amd import ops as O
    L, lib = _lib()
    a = [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in args]
    return getattr(lib, fn)(*a, O._stream())


def _run(fn, *args):
    _lib()[0].check(_call(fn, *args), fn)


def _refused(fn, *args):
    """The call returns LL_ERR_INVALID_ARG and leaves a message that names the entry point."""
    rc = _call(fn, *args)
    msg = _lib()[1].ll_last_error().decode()
    assert rc == INVALID and fn in msg, (fn, rc, msg)


def _nan16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(bf)


def _nan32(*shape):
    return torch.full(shape, NAN32, dtype=torch.int32, device=DEV).view(f32)


def _untouched(t):
    if t.dtype == f32:
        return bool((t.contiguous().view(torch.int32) == NAN32).all())
    return bool((t.contiguous().view(torch.int16) == NAN16).all())


def _guard_in(t, pad=3):
    """t [rows, cols] on the device, followed by `pad` rows of NaN: a read past the last row reaches the output."""
    t = t.reshape(-1, t.shape[-1])
    buf = torch.full((t.shape[0] + pad, t.shape[1]), float("nan"), dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t.to(DEV)
    return buf


def _same(got, want, what):
    """Bit comparison of a device tensor with the host's expected tensor."""
    g, w = got.detach().cpu().contiguous(), want.contiguous()
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape)
    it = torch.int32 if g.dtype == f32 else torch.int16
    ne = g.view(it) != w.view(it)
    if bool(ne.any()):
        g2, w2, n2 = g.reshape(-1, g.shape[-1]), w.reshape(-1, w.shape[-1]), ne.reshape(-1, ne.shape[-1])
        r = n2.any(-1).nonzero().flatten()
        c = n2.any(0).nonzero().flatten()
        i, j = int(r[0]), int(n2[r[0]].nonzero()[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ; rows {r[:8].tolist()}, columns {c[:8].tolist()}; "
                             f"first got {float(g2[i, j])} want {float(w2[i, j])}")


def _mod_inputs(B, F, C, seed):
    return E.hnorm((B, F, 6, C), seed, 0.5), E.hnorm((6, C), seed + 1, 1 / math.sqrt(C))


# ---- 2. row kernels at every dispatch instance --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", E.WIDTHS)
def test_ln_modulate(C):
    """ll_ln_modulate with mod (the per-row sum) and with mod = NULL on the precomputed table."""
    for B, F, fl in E.ROW_GEOS:
        rows, L = B * F * fl, F * fl
        x = E.exact_rows(rows, C, seed=C + B)[0].view(B, L, C)
        e, mod = _mod_inputs(B, F, C, C)
        pre = E.modulation_table_host(e.view(B * F, 6, C), mod.view(1, 6, C))[0]       # host chain, not ll_modulation_table's output
        xd, ed, md, pd = _guard_in(x), _guard_in(e), mod.to(DEV), _guard_in(pre)
        for sh, sc in E.MOD_PAIRS:
            want = E.ln_modulate_host(x, e, mod, sh, sc, F)
            for ee, mm, what in ((ed, md, "mod"), (pd, None, "table")):
                out = _nan16(rows + 3, C)
                _run("ll_ln_modulate", xd, out, ee, mm, 6, sh, sc, B, L, C, F, E.EPS)
                torch.cuda.synchronize()
                assert _untouched(out[rows:]), f"wrote past row {rows} (C {C})"
                _same(out[:rows], want, f"ln_modulate {what} C {C} rows {rows} idx {sh},{sc}")


@pytest.mark.parametrize("C", E.WIDTHS)
def test_ln_modulate_tab(C):
    for B, F, fl in E.ROW_GEOS:
        rows, L = B * F * fl, F * fl
        x = E.exact_rows(rows, C, seed=C + B)[0].view(B, L, C)
        e, mod = _mod_inputs(B, F, C, C)
        tab = E.modulation_table_f32_host(e.view(B * F, 6, C), mod.view(1, 6, C), 0b010010)[0]
        xd, td = _guard_in(x), _guard_in(tab)
        for sh, sc in E.MOD_PAIRS:
            out = _nan16(rows + 3, C)
            _run("ll_ln_modulate_tab", xd, out, None, None, td, 6, sh, sc, B, L, C, F, E.EPS)
            torch.cuda.synchronize()
            assert _untouched(out[rows:]), f"wrote past row {rows} (C {C})"
            _same(out[:rows], E.ln_modulate_tab_host(x, tab, sh, sc, F), f"ln_modulate_tab C {C} rows {rows} idx {sh},{sc}")


@pytest.mark.parametrize("C", E.WIDTHS)
def test_layernorm_affine(C):
    w, b = E.hnorm((C,), C + 2, 0.1, 1.0), E.hnorm((C,), C + 3, 0.1)
    wd, bd = _guard_in(w.view(1, C), 1), _guard_in(b.view(1, C), 1)
    for rows in (1, 5, 42):
        x = E.exact_rows(rows, C, seed=C + rows)[0]
        out = _nan16(rows + 3, C)
        _run("ll_layernorm_affine", _guard_in(x), wd, bd, out, rows, C, E.EPS)
        torch.cuda.synchronize()
        assert _untouched(out[rows:]), f"wrote past row {rows} (C {C})"
        _same(out[:rows], E.layernorm_affine_host(x, w, b), f"layernorm_affine C {C} rows {rows}")


@pytest.mark.parametrize("C", E.WIDTHS)
def test_rmsnorm(C):
    """ldo = C + 8 always; x contiguous and as the left half of rows of 2C whose right half is NaN."""
    w = E.hnorm((C,), C + 2, 0.1, 1.0)
    wd = _guard_in(w.view(1, C), 1)
    for rows in (1, 5, 42):
        x = E.exact_rows(rows, C, seed=C + rows + 1, means=0.0)[0]
        want = E.rmsnorm_host(x, w)
        wide = torch.full((rows + 3, 2 * C), float("nan"), dtype=bf, device=DEV)
        wide[:rows, :C] = x.to(DEV)
        for xd, ldx in ((_guard_in(x), C), (wide, 2 * C)):
            out = _nan16(rows + 3, C + 8)
            _run("ll_rmsnorm", xd, wd, out, rows, C, ldx, C + 8, E.EPS)
            torch.cuda.synchronize()
            assert _untouched(out[rows:]) and _untouched(out[:rows, C:]), f"wrote outside [rows, C] (C {C}, ldx {ldx})"
            _same(out[:rows, :C], want, f"rmsnorm C {C} rows {rows} ldx {ldx}")


@pytest.mark.parametrize("NL,BF,nmod,C,mask", E.MOD_TABLE_SHAPES)
def test_modulation_tables(NL, BF, nmod, C, mask):
    e, mods = E.hnorm((BF, nmod, C), C + 7, 0.5), E.hnorm((NL, nmod, C), C + 8, 0.1)
    n = NL * BF * nmod * C
    ed, md = _guard_in(e.view(BF, nmod * C)), _guard_in(mods.view(NL, nmod * C))
    out = _nan16(n + 64)
    _run("ll_modulation_table", ed, md, out, NL, BF, nmod, C)
    out32 = _nan32(n + 64)
    _run("ll_modulation_table_f32", ed, md, out32, NL, BF, nmod, C, mask)
    torch.cuda.synchronize()
    assert _untouched(out[n:]) and _untouched(out32[n:])
    _same(out[:n].view(NL, BF, nmod, C), E.modulation_table_host(e, mods), "modulation_table")
    _same(out32[:n].view(NL, BF, nmod, C), E.modulation_table_f32_host(e, mods, mask), "modulation_table_f32")


QK_CASES = [(C, D, sf, kind) for C, D in E.QK_SHAPES for sf in E.QK_START_FRAMES for kind in ("hash", "model")]


@pytest.mark.parametrize("C,D,sf,kind", QK_CASES)
def test_qk_norm_rope_kv_store(C, D, sf, kind):
    d = E.QKData(C, D)
    B, L, rows = d.B, d.L, d.B * d.L
    rf, rhw = d.tables(kind, sf)
    assert rf.shape[0] == sf + d.F and rhw.shape[0] == d.fl           # NaN directly after the last row a case may read
    rfd, rhwd = _guard_in(rf.view(rf.shape[0], -1)), _guard_in(rhw.view(d.fl, -1))
    want_q, want_k = d.expected(kind, sf)
    v = d.v.view(B, L, C)
    qkv, wq, wk = _guard_in(d.qkv), _guard_in(d.wq.view(1, C), 1), _guard_in(d.wk.view(1, C), 1)
    G = 3
    for S, ws, ro, wl in E.QK_WINDOWS:
        empty = torch.full((B, S, C), NAN16, dtype=torch.int16).view(bf)
        for with_v in (True, False):
            q_out = _nan16(rows + 3, C)
            kb, vb = _nan16(G + B * S + G, C), _nan16(G + B * S + G, C)
            ck, cv = kb[G:G + B * S], vb[G:G + B * S]
            _run("ll_qk_norm_rope_kv_store", qkv, wq, wk, rfd, rhwd, q_out, ck, cv if with_v else None, B, L, C, D, d.fl, sf, S, ws, ro,
                 wl, E.EPS)
            torch.cuda.synchronize()
            what = f"C {C} head {D} start {sf} {kind} window ({S}, {ws}, {ro}, {wl}) v {with_v}"
            assert _untouched(q_out[rows:]) and _untouched(kb[:G]) and _untouched(kb[-G:]) and _untouched(vb[:G]) and _untouched(vb[-G:]), what
            _same(q_out[:rows], want_q, "q_out " + what)
            _same(ck.view(B, S, C), E.kv_insert_host(empty, want_k, S, ws, ro, wl), "cache k " + what)      # every slot outside the window: NAN16
            if with_v:
                _same(cv.view(B, S, C), E.kv_insert_host(empty, v, S, ws, ro, wl), "cache v " + what)
            else:
                assert _untouched(vb), "cache_v = NULL: V must not be written " + what


def test_row_kernels_refuse_bad_shapes():
    s = _nan16(1 << 20)               # every pointer: large enough for any of the shapes below, so a launch that slipped through shows
    tab = _nan32(1 << 18)
    for C in (2056, 12):
        _refused("ll_ln_modulate", s, s, s, s, 6, 0, 1, 1, 2, C, 1, E.EPS)
        _refused("ll_ln_modulate_tab", s, s, None, None, tab, 6, 0, 1, 1, 2, C, 1, E.EPS)
        _refused("ll_layernorm_affine", s, s, s, s, 2, C, E.EPS)
        _refused("ll_rmsnorm", s, s, s, 2, C, C, C, E.EPS)
        _refused("ll_qk_norm_rope_kv_store", s, s, s, tab, tab, s, s, s, 1, 2, C, 4 if C == 12 else 8, 1, 0, 4, 0, 0, 2, E.EPS)
    _refused("ll_rmsnorm", s, s, s, 2, 256, 256, 248, E.EPS)                                                  # ldo < C
    qk = lambda *a: _refused("ll_qk_norm_rope_kv_store", s, s, s, tab, tab, s, s, s, *a, E.EPS)
    #  B, L, C, head_dim, frame_len, start_frame, S, write_start, roped_offset, write_len
    qk(1, 2, 256, 96, 1, 0, 4, 0, 0, 2)            # head_dim does not divide C
    qk(1, 2, 256, 128, 1, 1023, 4, 0, 0, 2)        # start_frame + F = 1025
    qk(1, 2, 256, 128, 1, 0, 4, 3, 0, 2)           # the window ends past S
    qk(1, 2, 256, 128, 1, 0, 4, 0, 1, 2)           # ... past L
    torch.cuda.synchronize()
    assert _untouched(s) and _untouched(tab)


# ---- 3. cache and latent kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,C,dst,src,n", E.KV_ROLL_CASES)
def test_kv_roll(B, S, C, dst, src, n):
    G = 3
    k0, v0 = E.hash_bf16_bits((B, S, C), 21).view(bf), E.hash_bf16_bits((B, S, C), 22).view(bf)
    kb, vb = _nan16(G + B * S + G, C), _nan16(G + B * S + G, C)
    kb[G:G + B * S] = k0.view(B * S, C).to(DEV)
    vb[G:G + B * S] = v0.view(B * S, C).to(DEV)
    _run("ll_kv_roll", kb[G:], vb[G:], B, S, C, dst, src, n)
    torch.cuda.synchronize()
    assert _untouched(kb[:G]) and _untouched(kb[-G:]) and _untouched(vb[:G]) and _untouched(vb[-G:])
    _same(kb[G:G + B * S].view(B, S, C), E.kv_roll_host(k0, dst, src, n), "k")
    _same(vb[G:G + B * S].view(B, S, C), E.kv_roll_host(v0, dst, src, n), "v")


def test_kv_roll_refuses_dst_at_or_behind_src():
    s = _nan16(4096)
    _refused("ll_kv_roll", s, s, 1, 16, 8, 4, 4, 2)
    _refused("ll_kv_roll", s, s, 1, 16, 8, 5, 4, 2)
    _refused("ll_kv_roll", s, s, 1, 16, 12, 2, 4, 2)
    torch.cuda.synchronize()
    assert _untouched(s)


def _sigmas(n, rot):
    vals = [E.SIGMA_GENERIC, 0.0, 1.0]
    return torch.tensor([vals[(i + rot) % 3] for i in range(n)], dtype=f32)


@pytest.mark.parametrize("B,F,C,H,W", E.LATENT_SHAPES)
def test_patchify_and_unpatchify_x0(B, F, C, H, W):
    x = E.hnorm((B, F, C, H, W), C + H, 1.0)
    n = x.numel()
    out = _nan16(n + 64)
    _run("ll_patchify", _guard_in(x.view(-1, W)), out, B, F, C, H, W)
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    _same(out[:n].view(B, F * (H // 2) * (W // 2), C * 4), E.patchify_host(x), "patchify")
    head = E.hnorm((B, F * (H // 2) * (W // 2), 4 * C), C + H + 1, 1.0)
    want_flow = E.unpatchify_host(head, B, F, C, H, W)
    for rot in range(3):                                   # every frame sees sigma 0, 1 and the generic value
        sigma = _sigmas(B * F, rot)
        flow, x0 = _nan16(n + 64), _nan16(n + 64)
        _run("ll_unpatchify_x0", _guard_in(head.view(-1, 4 * C)), _guard_in(x.view(-1, W)), sigma.to(DEV), flow, x0, B, F, C, H, W)
        torch.cuda.synchronize()
        assert _untouched(flow[n:]) and _untouched(x0[n:])
        _same(flow[:n].view(B, F, C, H, W), want_flow, "flow")
        _same(x0[:n].view(B, F, C, H, W), E.x0_host(x, want_flow, sigma.view(B, F)), f"x0 (sigma rotation {rot})")
    s = _nan16(4096)
    for h, w in ((3, 4), (4, 3)):
        _refused("ll_patchify", s, s, 1, 1, 1, h, w)
        _refused("ll_unpatchify_x0", s, s, s, s, s, 1, 1, 1, h, w)
    torch.cuda.synchronize()
    assert _untouched(s)


@pytest.mark.parametrize("N,inner", E.ADD_NOISE_SHAPES)
def test_add_noise(N, inner):
    x0, nz = E.hnorm((N, inner), inner, 1.0), E.hnorm((N, inner), inner + 1, 1.0)
    for rot in range(3):
        sigma = _sigmas(N, rot)
        out = _nan16(N * inner + 64)
        _run("ll_add_noise", _guard_in(x0), _guard_in(nz), sigma.to(DEV), out, N, inner)
        torch.cuda.synchronize()
        assert _untouched(out[N * inner:])
        _same(out[:N * inner].view(N, inner), E.add_noise_host(x0, nz, sigma), f"add_noise (sigma rotation {rot})")
    s = _nan16(4096)
    _refused("ll_add_noise", s, s, s, s, 1, 12)
    torch.cuda.synchronize()
    assert _untouched(s)


@pytest.mark.parametrize("dim,ts", E.SINUSOID_CASES)
def test_sinusoid(dim, ts):
    t = torch.tensor(ts, dtype=f32)
    n, half = len(ts), dim // 2
    out = _nan16(n * dim + 64)
    _run("ll_sinusoid", t.to(DEV), out, n, dim)
    torch.cuda.synchronize()
    assert _untouched(out[n * dim:])
    got, want = out[:n * dim].view(n, dim).cpu(), E.sinusoid_host(t, dim).to(bf)
    for r in range(n):
        for lo, name in ((0, "cos"), (half, "sin")):
            assert_bf16_close(got[r, lo:lo + half], want[r, lo:lo + half], 1, 0.98, f"{name} half of row {r} (t {ts[r]}, dim {dim})")
        if ts[r] == 0.0:
            _same(got[r], torch.cat([torch.ones(half), torch.zeros(half)]).to(bf), "t = 0")
    s = _nan16(4096)
    _refused("ll_sinusoid", s, s, 1, 3)
    torch.cuda.synchronize()
    assert _untouched(s)


@pytest.mark.parametrize("name", ["real", "n5", "n64", "n65", "repeat"])
def test_sigma_lookup(name):
    """Against torch.argmin of fp64 distances.  Directly after each table lie 64 entries that hold the exact value of the query below the
    table's range (and a sigma of 777): a lane that read past n_table would win with distance 0."""
    ts, sg = E.sigma_tables()[name]
    q = E.sigma_queries(ts)
    n, nt = q.numel(), ts.numel()
    tsd = torch.cat([ts, torch.full((64,), float(ts.min()) - 0.5)]).to(DEV)
    sgd = torch.cat([sg, torch.full((64,), 777.0)]).to(DEV)
    out = _nan32(n + 3)
    _run("ll_sigma_lookup", q.to(DEV), tsd, sgd, out, n, nt)
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    _same(out[:n], E.sigma_lookup_host(q, ts, sg), f"sigma_lookup {name}")
    assert float(out[n - 1]) == float(sg[0]) and math.isnan(float(q[-1]))       # the NaN query: sigmas[0]


# ---- 4. ll_linear_small ---------------------------------------------------------------------------------------------------------------------
def _linear(x, w, bias, M, N, K, act_in, act_out):
    """x is followed by NaN rows up to row 8 and beyond, w by NaN rows; the output is a flat NaN field."""
    out = _nan16(M * N + 64)
    _run("ll_linear_small", _guard_in(x, 9), _guard_in(w, 4), _guard_in(bias.view(1, N), 1), out, M, N, K, act_in, act_out)
    torch.cuda.synchronize()
    assert _untouched(out[M * N:]), f"wrote past [M, N] ({M}, {N}, {K})"
    return out[:M * N].view(M, N)


# act_out = 1, share of outputs bit-identical to fp64 SiLU rounded once, over every (M, N) of a K (3180 outputs each):
#   torch's fp32 SiLU rounded to bf16 (measured in tests/test_rows_edges_host.py): 1.0000 at every K, 0 ulp at the worst
#   ll_linear_small (v_exp_f32 / v_rcp_f32 form): printed by the test below (pytest -s); it must not fall more than
#   rows_exact.SILU_SHARE_SLACK below torch's share of the same run
@pytest.mark.parametrize("K", E.LINEAR_K)
def test_linear_small(K):
    got_s, want_s, torch_s = [], [], []
    for M in E.LINEAR_M:
        for N in E.LINEAR_N:
            d = E.LinearData(M, N, K)
            _same(_linear(d.x, d.w, d.bias, M, N, K, 0, 0), d.pre, f"linear_small M {M} N {N} K {K}")
            got_s.append(_linear(d.x, d.w, d.bias, M, N, K, 0, 1).cpu().flatten())
            want_s.append(d.silu64().to(bf).flatten())
            torch_s.append(torch.nn.functional.silu(d.pre.to(f32)).to(bf).flatten())
    got, want, tor = torch.cat(got_s), torch.cat(want_s), torch.cat(torch_s)
    dist = bf16_ulp_distance(got, want)
    share, tshare = float((dist == 0).float().mean()), float((bf16_ulp_distance(tor, want) == 0).float().mean())
    print(f"act_out = 1, K = {K}: kernel {share:.4f} exact (worst {int(dist.max())} ulp), torch {tshare:.4f}")
    assert int(dist.max()) <= 1, f"act_out: {int((dist > 1).sum())} outputs further than 1 ulp from fp64 SiLU rounded once"
    assert share >= tshare - E.SILU_SHARE_SLACK, (share, tshare)


@pytest.mark.parametrize("K", E.LINEAR_ACT_IN_K)
def test_linear_small_act_in(K):
    for M in E.LINEAR_M:
        for N in E.LINEAR_N:
            d = E.LinearActInData(M, N, K)
            _same(_linear(d.x, d.w, d.bias, M, N, K, 1, 0), d.want, f"linear_small act_in M {M} N {N} K {K}")


def test_linear_small_refusals():
    s = _nan16(1 << 16)
    _refused("ll_linear_small", s, s, s, s, 9, 4, 8, 0, 0)
    _refused("ll_linear_small", s, s, s, s, 2, 4, 12, 0, 0)
    torch.cuda.synchronize()
    assert _untouched(s)
