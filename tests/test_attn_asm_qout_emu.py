"""The quantised-output forms of the generated self-attention kernel (gen/attn_asm_gen.py, generate(out="mx" | "mx6" | "mx4")) on
the CPU emulator: the codes and E8M0 scales they write are, bit for bit, the host quantisers (mx_ref / mx6_ref / mx4_ref) applied to
the bf16 rows the plain text writes for the same inputs; nothing outside the head's code bytes and four scale bytes is touched; the
edge values of the scale rule and of the code rounding are forced through one-hot attention rows (the output row IS a chosen V row);
and generate() without `out` still emits the parent's text."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from attn_qout_emu import FMTS, STEP, D, G, bf16_bits, bf16_val, expected, one_hot_case, run

# sha256 of generate("buffer", "LLB") and generate("buffer", "LLBN", False, True) at the commit before the `out` argument existed
PARENT_SHA = {"plain": "6e0c963ee6da6553cad089be080f05185a2166c0dcc8e62f47cca4fab71498b0",
              "qnorm": "84569faef81daaf6fac7b1e6e29f7e3596243356aa494058b5ef6e7553237016"}


@pytest.fixture(scope="module")
def texts():
    t = {None: G.generate("buffer", "LLB")}
    for f in FMTS:
        t[f] = G.generate("buffer", "LLB" + f.upper(), out=f)
    return t


def random_case(rows_valid, nkeys, seed, nheads=2, kstart=3):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((rows_valid, nheads, D)).astype(np.float32)
    k = rng.standard_normal((kstart + nkeys, nheads, D)).astype(np.float32)
    # V with block maxima over many binades, exact zeros and whole zero blocks
    v = (rng.standard_normal((kstart + nkeys, nheads, D)) * np.exp2(rng.integers(-6, 5, (kstart + nkeys, nheads, 4)).repeat(32, -1))).astype(np.float32)
    v[rng.random(v.shape) < 0.05] = 0.0
    return bf16_bits(q), bf16_bits(k), bf16_bits(v)


@pytest.mark.parametrize("fmt", FMTS)
def test_text_is_lint_clean_and_assembles(texts, fmt, tmp_path):
    assert G.lint(texts[fmt]) == []
    clang = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(clang):
        pytest.skip("no ROCm assembler here")
    src = tmp_path / "k.s"
    src.write_text('.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n.text\nkernel:\n' + texts[fmt])
    r = subprocess.run([clang, "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", str(src), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:2000]


@pytest.mark.parametrize("fmt", FMTS)
def test_prologue_and_loop_are_the_plain_text(texts, fmt):
    """only the text after the epilogue label differs (the prefix aside)"""
    a = texts[None].split("LLB_EPILOGUE:")[0]
    b = texts[fmt].replace("LLB" + fmt.upper() + "_", "LLB_").split("LLB_EPILOGUE:")[0]
    assert a == b


@pytest.fixture(scope="module")
def plain_outputs(texts):
    """the plain text's bf16 rows per (geometry, mode): computed once, shared by the three formats"""
    cache = {}

    def get(key, mode, args):
        if (key, mode) not in cache:
            cache[(key, mode)] = run(texts[None], mode, *args)
        return cache[(key, mode)]
    return get


GEOMS = {"full_ragged_keys": (256, 6 * 64 + 20, 0), "partial_wave_idle_waves": (72, 5 * 64, 3)}


@pytest.mark.parametrize("mode", ["lazy", "eager"])
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("fmt", FMTS)
def test_random_data_is_the_quantiser_of_the_plain_rows(texts, plain_outputs, fmt, geom, mode):
    rows, nkeys, seed = GEOMS[geom]
    nheads, head, kstart = 2, 1, 3
    q, k, v = random_case(rows, nkeys, seed, nheads, kstart)
    args = (q, k, v, rows, nkeys, nheads, head, kstart)
    out_bits = plain_outputs(geom, mode, args)
    assert np.isfinite(bf16_val(out_bits)).all()
    codes, scales = run(texts[fmt], mode, *args, fmt=fmt)
    wc, ws = expected(fmt, out_bits, nheads, head)
    assert np.array_equal(scales, ws), np.argwhere(scales != ws)[:8]
    assert np.array_equal(codes, wc), np.argwhere(codes != wc)[:8]


# ---- edge values through one-hot rows -----------------------------------------------------------------------------------------

def _frexp_bits(amax):
    m, p = np.frexp(amax.astype(np.float64))
    return m, p


@pytest.mark.parametrize("fmt", FMTS)
def test_edge_values_through_one_hot_rows(texts, fmt):
    nheads, head, kstart = 2, 1, 3
    q, k, v, rows, nkeys, pos = one_hot_case(fmt, nheads=nheads, head=head, kstart=kstart)
    args = (q, k, v, rows, nkeys, nheads, head, kstart)
    out_bits = run(texts[None], "lazy", *args)
    # the construction holds: every row but row 0 is its key's V row, row 0 is half of its first key's
    assert np.array_equal(out_bits[1:], v[kstart + pos[1:rows], head])
    x = bf16_val(out_bits).astype(np.float64).reshape(rows, 4, 32)
    amax = np.abs(x).max(-1)
    m, p = np.frexp(amax)
    thr = {"mx": 0.875, "mx6": 0.9375, "mx4": 0.75}[fmt]
    ulp = 2.0 ** -8                                        # of a bf16 mantissa in frexp's [0.5, 1)
    sub = {"mx": 9, "mx6": 3, "mx4": 3}[fmt]
    e = np.clip(np.where(amax > 0, p - sub + (m > thr), 0), -127, 127)
    vs = x * np.exp2(-e.astype(np.float64))[..., None]                 # the scaled values the codes are taken of
    st = STEP[fmt]
    occurs = {
        "an all-zero block": (amax == 0).any(),
        "amax exactly at the largest code": ((m == thr) & (amax > 0)).any(),
        "amax one bf16 ulp above it": (m == thr + ulp).any(),
        "amax one bf16 ulp below it": (m == thr - ulp).any(),
        "-0.0": (out_bits == 0x8000).any(),
        "a value that rounds to the smallest subnormal code": ((np.abs(vs) > 0.5 * st) & (np.abs(vs) < st)).any(),
        "a non-zero value that rounds to zero": ((np.abs(vs) > 0) & (np.abs(vs) < 0.5 * st)).any(),
        "a negative value that rounds to zero": ((vs < 0) & (np.abs(vs) < 0.5 * st)).any(),
        "a tie between zero and the smallest subnormal": (np.abs(vs) == 0.5 * st).any(),
        "a tie between two subnormal codes": (np.abs(vs) == 1.5 * st).any(),
        "a tie between two normal codes, even below": (np.abs(vs) == (1.25 if fmt == "mx4" else 1.0625)).any(),
        "a tie between two normal codes, even above": (np.abs(vs) == (1.75 if fmt == "mx4" else 1.1875)).any(),
        "amax 2^-130 (exponent clamped at -127)": ((amax == 2.0 ** -130) & (e == -127)).any(),
    }
    missing = [kk for kk, ok in occurs.items() if not ok]
    assert not missing, missing
    codes, scales = run(texts[fmt], "lazy", *args, fmt=fmt)
    wc, ws = expected(fmt, out_bits, nheads, head)
    assert (ws[:, 4 * head: 4 * head + 4] == 127).any() and (ws[:, 4 * head: 4 * head + 4] == 0).any()
    assert np.array_equal(scales, ws), np.argwhere(scales != ws)[:8]
    assert np.array_equal(codes, wc), np.argwhere(codes != wc)[:8]


def test_default_text_is_the_parents():
    assert hashlib.sha256(G.generate("buffer", "LLB").encode()).hexdigest() == PARENT_SHA["plain"]
    assert hashlib.sha256(G.generate("buffer", "LLBN", False, True).encode()).hexdigest() == PARENT_SHA["qnorm"]
    assert G.generate("buffer", "LLB", out=None) == G.generate("buffer", "LLB")
