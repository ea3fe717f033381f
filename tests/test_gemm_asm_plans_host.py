"""What ll_gemm_plan_epi, ll_gemm_ksplit_plan and ll_gemm_ssq_planes answer, held string for string to a recording of the library
as it was before the generated GEMMs' selection moved into one function (gemm_asm.hip: gemm_asm_pick, used by launch and plan).
tests/golden/gemm_asm_plans.json was written by record() below from that earlier library and is not to be re-recorded from a later
one: a difference is a change of route or of a plan string.

Section `host` is the library without a device (0 compute units: classic kernels only); section `gpu` (tests/
test_gemm_asm_plans_gpu.py) holds the launches of more tiles than compute units, where the persistent kernels appear.  A set is a
tuning (gemm_asm, gemm_asm_mfma16) and a grid M x N x K x epilogue x int8 x plain; `plan` holds one index into `strings` per grid
point (itertools.product order), `ksplit` and `ssq` one int per M x N x K.

The sets of `host` and the branches of the width rule (gemm_asm.hip: ga_width) they are there for:
  shipped       gemm_asm 35, mask 511, the full shape grid: every bf16 classic _m16 kernel (224 GELU at N = 8960; 192 at N = 2304, 4608 and
                for the QKV form plain = 2; 256 at M <= 1024, N >= 16384; the three 128-wide ones), K % 64 (K = 64 is also K < 256),
                K < 256 (192), N % 128 (200), N > 2048 with M > 1024 (M = 1025, N = 3584), plain = 0, the QKV form refused where the V
                third starts off a tile boundary (N = 1536) or N % 192 != 0, int8 calls on the HIP kernels (bit 4 clear)
  w8a8          gemm_asm 51: the five gemm_asmq_* kernels, K % 128 (64, 192, 448), K < 512 (256), no 256-wide kernel (N = 20480: HIP),
                128-wide only up to N = 2048 whatever M
  edges         gemm_asm 51: M <= 0, the 32-bit byte-offset bounds (bf16 K = 4194304 refused, 4194240 taken; int8 K = 8388608 refused,
                8388480 taken), an epilogue code outside LL_EPI_* (int8: the 128-wide residual kernel; bf16: HIP)
  gemm_asm=*    0 (all HIP), 1 and 3 (as 35 without a device), 5 (GELU left out), 9 (everything but GELU left out), 19 (W8A8 too) on a
                reduced grid with one shape per width and per refusal
  mfma16=*      mask 0 (every 32x32x16 kernel) and each single bit on the same reduced grid: the bit of each kernel
Two refusals cannot be reached through these entry points and are held by the GPU suites' launches alone: ldx % 8 (the plan passes
ldx = K) and the gate-residual epilogue without a frame length (the plan passes 1).  The row-sum and split-K partial kernels have no
plan string; ll_gemm_ssq_planes and ll_gemm_ksplit_plan are their selection."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_asm_plans.json")
AXES = ("M", "N", "K", "epi", "int8", "plain")

FULL = dict(M=[1, 256, 257, 1024, 1025, 4680], N=[128, 200, 384, 1536, 2048, 2304, 3584, 4608, 8960, 16384, 20480],
            K=[64, 192, 256, 448, 512, 1536], epi=[0, 1, 2, 3], int8=[0, 1], plain=[0, 1, 2])
REDUCED = dict(FULL, M=[256, 1025], N=[200, 384, 1536, 2304, 8960, 20480], K=[192, 512])
EDGES = dict(M=[-1, 0, 256], N=[128, 2304], K=[256, 512, 4194240, 4194304, 8388480, 8388608], epi=[0, 1, 2, 3, 7], int8=[0, 1], plain=[0, 1, 2])
MASKS = [0, 511] + [1 << b for b in range(9)]
HOST_SETS = ([dict(name="shipped", gemm_asm=35, mfma16=511, **FULL), dict(name="w8a8", gemm_asm=51, mfma16=511, **dict(FULL, int8=[1])),
              dict(name="edges", gemm_asm=51, mfma16=511, **EDGES)]
             + [dict(name=f"gemm_asm={g}", gemm_asm=g, mfma16=511, **REDUCED) for g in (0, 1, 3, 5, 9, 19)]
             + [dict(name=f"mfma16={m}", gemm_asm=35, mfma16=m, **REDUCED) for m in MASKS if m != 511])
# more tiles than compute units (K = 256), every mask with and without the persistent form; W8A8 never persistent; the split-K plan
GPU_SHAPES = dict(M=[1352, 2900, 4200, 4680, 9360], N=[1536, 2048, 4608, 9216, 10752, 8960], K=[256], epi=[0, 1, 2, 3], int8=[0], plain=[1, 2])
GPU_SETS = ([dict(name=f"gemm_asm={g} mfma16={m}", gemm_asm=g, mfma16=m, **GPU_SHAPES) for g in (35, 3) for m in MASKS]
            + [dict(name="w8a8", gemm_asm=51, mfma16=511, **dict(GPU_SHAPES, K=[512], int8=[1])),
               dict(name="ksplit", gemm_asm=35, mfma16=511, **dict(FULL, K=[512, 1536, 4096], epi=[0, 3], int8=[0], plain=[1]))])


def _lib():
    from longlive_amd import _lib as L
    return L.load()


def answers(lib, s):
    """(plan strings, ksplit ints, ssq ints) of one set under its tuning; the shipped tuning is restored afterwards."""
    buf = ctypes.create_string_buffer(512)
    try:
        assert lib.ll_set_tuning(b"gemm_asm", s["gemm_asm"]) == 0 and lib.ll_set_tuning(b"gemm_asm_mfma16", s["mfma16"]) == 0
        plans = []
        for M, N, K, epi, int8, plain in itertools.product(*(s[a] for a in AXES)):
            assert lib.ll_gemm_plan_epi(M, N, K, int8, epi, plain, buf, 512) == 0
            plans.append(buf.value.decode())
        shapes = list(itertools.product(s["M"], s["N"], s["K"]))
        return plans, [lib.ll_gemm_ksplit_plan(*mnk) for mnk in shapes], [lib.ll_gemm_ssq_planes(*mnk) for mnk in shapes]
    finally:
        lib.ll_set_tuning(b"gemm_asm", 35)
        lib.ll_set_tuning(b"gemm_asm_mfma16", -1)


def device_cus(lib):
    """Compute units the library sees (0 = no device), read off the persistent plan of a launch with more tiles than any device has
    compute units."""
    buf = ctypes.create_string_buffer(512)
    assert lib.ll_gemm_plan_epi(1 << 20, 2048, 256, 0, 0, 1, buf, 512) == 0
    words = buf.value.decode().split()
    return int(words[words.index("persistent") - 1]) if "persistent" in words else 0


def record(section, sets):
    """Writes one section of the golden file from the library LONGLIVE_HIP_LIB names.  Run by hand, once, against the library the
    later ones are held to:  LONGLIVE_HIP_LIB=<that library> python tests/test_gemm_asm_plans_host.py record host|gpu"""
    lib = _lib()
    doc = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {"strings": []}
    index = {t: i for i, t in enumerate(doc["strings"])}
    out = []
    for s in sets:
        plans, ksplit, ssq = answers(lib, s)
        for t in plans:
            index.setdefault(t, len(index))
        out.append(dict(s, plan=[index[t] for t in plans], ksplit=ksplit, ssq=ssq))
    doc["strings"] = list(index)
    doc[section] = dict(cus=device_cus(lib), sets=out)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": ' + (json.dumps(v, separators=(",", ":")) if k != "strings" else
                                                  "[\n" + ",\n".join(json.dumps(t) for t in v) + "\n]") for k, v in doc.items()) + "\n}\n")


def mismatches(lib, section):
    """Every answer of a section that differs from the recording, as readable lines."""
    doc = json.load(open(GOLDEN))
    bad = []
    for s in doc[section]["sets"]:
        plans, ksplit, ssq = answers(lib, s)
        want = [doc["strings"][i] for i in s["plan"]]
        assert len(plans) == len(want) and len(ksplit) == len(s["ksplit"]) and len(ssq) == len(s["ssq"])
        for case, got, exp in zip(itertools.product(*(s[a] for a in AXES)), plans, want):
            if got != exp:
                bad.append(f"{s['name']} {dict(zip(AXES, case))}: {got!r}, recorded {exp!r}")
        for what, gots, exps in (("ksplit", ksplit, s["ksplit"]), ("ssq planes", ssq, s["ssq"])):
            for mnk, got, exp in zip(itertools.product(s["M"], s["N"], s["K"]), gots, exps):
                if got != exp:
                    bad.append(f"{s['name']} {what} {mnk}: {got}, recorded {exp}")
    return bad


def test_recorded_sets_are_the_documented_ones():
    doc = json.load(open(GOLDEN))
    strip = lambda sets: [{k: v for k, v in s.items() if k not in ("plan", "ksplit", "ssq")} for s in sets]
    assert strip(doc["host"]["sets"]) == HOST_SETS and strip(doc["gpu"]["sets"]) == GPU_SETS
    assert doc["host"]["cus"] == 0 and doc["gpu"]["cus"] >= 8
    used = {i for sec in ("host", "gpu") for s in doc[sec]["sets"] for i in s["plan"]}
    assert used == set(range(len(doc["strings"])))
    names = {t.split("<")[0] for t in doc["strings"]}
    family = [f"gemm_asm{p}_{k}{m}" for p in ("", "p") for m in ("", "_m16")
              for k in ("224_gelu", "192_bias", "128_bias", "128_gate_res", "128_res")]
    family += ["gemm_asm_256_bias", "gemm_asm_256_bias_m16"] + [f"gemm_asmq_{k}" for k in ("224_gelu", "192_bias", "128_bias", "128_gate_res", "128_res")]
    assert set(family) <= names, sorted(set(family) - names)          # every kernel that has a plan string is recorded at least once


def test_host_plans_equal_the_recording():
    """Without a device, in this process; where the library sees one, in a child process that hides it (the section is the library
    without a device, whatever machine the suite runs on)."""
    lib = _lib()
    if device_cus(lib) == 0:
        bad = mismatches(lib, "host")
    else:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "check", "host"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        bad = json.loads(r.stdout.splitlines()[-1])
    assert not bad, f"{len(bad)} answers differ from the recording, the first: " + "; ".join(bad[:5])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    mode, section = sys.argv[1:3]
    if mode == "record":
        record(section, HOST_SETS if section == "host" else GPU_SETS)
    else:
        lib = _lib()
        assert device_cus(lib) == 0, "the device is still visible"
        print(json.dumps(mismatches(lib, section)))
