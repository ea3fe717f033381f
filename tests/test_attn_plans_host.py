"""What the attention entry points answer without a device -- ll_flash_attn_plan, ll_flash_attn_q_ok / _q_plan, ll_flash_attn_qnorm_ok,
ll_flash_attn_mx_plan, and the refusals and early returns of the six launching entry points -- held byte for byte to a recording of the
library as it was before the route decision moved into one function (attention.hip: attn_pick, used by launch, plan and _ok).
tests/golden/attn_plans.json was written by tools/record_attn_goldens.py from that earlier library and is not to be re-recorded from a
later one: a difference is a change of route, of a plan string or of an error text.

The groups of cases and the branches they are there for:
  plan/full     the shipped tuning over the whole shape grid: the workgroup counts of every kernel (Lq at and around the 128- and
                256-row tiles, one and two batch elements, H = 17), two ranges (flash_attn_kernel<4>), adjacent ranges merged into one,
                n0 around the two-tile floor (127 / 128 / 129), the generated kernel's threshold (511 / 512 / 513) and the ping-pong
                threshold (1023 / 1024)
  plan/tuning   every tuning (attn_variant x attn_asm x attn_asm_min_keys x attn_pp_min_keys x attn_xcd) over all key ranges of a thinned
                (Lq, H, B) grid: variant 0 (always the simple kernel), 1 (no ping-pong, no generated kernel), attn_asm 0,
                attn_asm_min_keys below the two-tile floor (0, 64), at it (128) and above, attn_pp_min_keys 0 / 512 / 1024 with the
                generated kernel off, the placement suffix
  plan/bound    n0 * H * 128 * 2 bytes just below and at 2^31 (H = 17: 493447 keys taken, 493448 refused by the generated kernel)
  q             ll_flash_attn_q_ok and _q_plan for fmt 0..4 (0 and 4 refused), H odd and even, under variant x attn_asm x
                attn_asm_min_keys: ranges adjacent (merged), separated, reversed-adjacent (not merged), overlapping, negative, empty
  qnorm         ll_flash_attn_qnorm_ok for H = 0..17 (1 <= H <= 16) under the same tunings, nkeys around the floors and at the 2^31 bound
  mx_plan       ll_flash_attn_mx_plan: range starts that are and are not multiples of 32 (tiles start at the start rounded down), one
                and two ranges, adjacent ones merged
  refusals      one call per LL_REQUIRE of ll_flash_attn, _qnorm, _q, _mx, _mx_q and _q_plan that fails exactly that check, and their
                B == 0 / Lq == 0 / H == 0 early returns: (return code, ll_last_error()).  Every call has Lq = 0 or B = 0, so one that
                is not refused returns before any launch as well."""
import ctypes
import itertools
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plans.json")
DEFAULTS = dict(attn_variant=2, attn_asm=1, attn_asm_min_keys=512, attn_pp_min_keys=1024, attn_xcd=1)
KEYS = tuple(DEFAULTS)

N0 = [1, 64, 127, 128, 129, 511, 512, 513, 1023, 1024, 18720]
FULL = dict(Lq=[1, 128, 129, 256, 257, 4680], H=[1, 2, 12, 17], B=[1, 2], n0=N0, n1=[0, 1, 512], adjacent=[0, 1])
THIN = dict(FULL, Lq=[257, 4680], H=[12], B=[2])
BOUND = dict(Lq=[257], H=[16, 17], B=[1], n0=[493447, 493448, 524287, 524288], n1=[0], adjacent=[0])
AXES = ("Lq", "H", "B", "n0", "n1", "adjacent")
TUNINGS = [dict(zip(KEYS, t)) for t in itertools.product([0, 1, 2], [0, 1], [0, 64, 128, 512, 1024], [0, 512, 1024], [0, 1])]
ROUTE_TUNINGS = [dict(DEFAULTS, attn_variant=v, attn_asm=a, attn_asm_min_keys=m) for v in (0, 1, 2) for a in (0, 1)
                 for m in (0, 64, 128, 512, 1024)]
PLAN_SETS = ([dict(name="full", tuning=DEFAULTS, **FULL), dict(name="bound", tuning=DEFAULTS, **BOUND)]
             + [dict(name="tuning", tuning=t, **THIN) for t in TUNINGS])
# (s0, n0, s1, n1): one range; adjacent; separated; reversed-adjacent; reversed-separated; overlapping; contained; negative start;
# negative second start; empty first; negative second length; short ranges that only reach the floor merged; long ranges
Q_RANGES = [(0, 512, 0, 0), (0, 256, 256, 256), (0, 256, 300, 256), (256, 256, 0, 256), (600, 256, 0, 256), (0, 512, 256, 512),
            (0, 1024, 100, 10), (-1, 512, 0, 0), (0, 512, -1, 512), (0, 0, 0, 512), (0, 512, 512, -1), (3, 64, 67, 64), (7, 127, 0, 0),
            (7, 128, 0, 0), (0, 18720, 0, 0)]
Q_CASES = list(itertools.product([0, 1, 2, 3, 4], [1, 2, 12, 17], Q_RANGES))
QNORM_CASES = list(itertools.product(range(18), [1, 127, 128, 511, 512, 1024, 524287, 524288]))
MX_PLAN_CASES = list(itertools.product([1, 128, 129, 4680], [1, 12], [1, 2],
                                       [(0, 40, 70, 130), (0, 40, 40, 160), (32, 64, 0, 0), (33, 64, 0, 0), (31, 1, 0, 0), (5, 59, 96, 33),
                                        (5, 59, 97, 200), (70, 130, 0, 40), (0, 9360, 0, 0), (3, 4680, 4700, 4660)]))

_P = 4096       # what the dummy pointers of the refused calls hold: never dereferenced
_S = 128 ** -0.5
# the valid argument lists the refused calls differ from in the named fields (B = 2 ... but Lq = 0: see the module docstring)
BASE = {
    "ll_flash_attn": dict(q=_P, k=_P, v=_P, out=_P, B=2, Lq=0, H=2, ldq=256, ldo=256, ldk=256, kbs=1 << 20, s0=0, n0=512, s1=0, n1=0,
                          scale=_S, stream=0),
    "ll_flash_attn_qnorm": dict(q=_P, ssq=_P, norm_w=_P, eps=1e-6, k=_P, v=_P, out=_P, B=2, Lq=0, H=2, ldq=256, ldo=256, ldk=256,
                                kbs=1 << 20, key_start=0, nkeys=512, scale=_S, stream=0),
    "ll_flash_attn_q": dict(fmt=1, q=_P, k=_P, v=_P, codes=_P, scales=_P, B=2, Lq=0, H=2, ldq=256, ldc=256, lds=8, ldk=256, kbs=1 << 20,
                            s0=0, n0=512, s1=0, n1=0, scale=_S, stream=0),
    "ll_flash_attn_mx": dict(q=_P, kq=_P, ks=_P, vq=_P, vs=_P, out=_P, B=2, Lq=0, H=2, head_dim=128, ldq=256, ldo=256, S=200, S32=224,
                             s0=0, n0=40, s1=70, n1=130, scale=_S, stream=0),
    "ll_flash_attn_mx_q": dict(fmt=1, q=_P, kq=_P, ks=_P, vq=_P, vs=_P, codes=_P, scales=_P, B=2, Lq=0, H=2, head_dim=128, ldq=256,
                               ldc=256, lds=8, S=200, S32=224, s0=0, n0=40, s1=70, n1=130, scale=_S, stream=0),
}
_SEGS_MX = [dict(S32=200), dict(S=0, S32=0), dict(n0=0), dict(s0=-1), dict(s0=190, n0=40), dict(n1=-1), dict(s1=-1), dict(s1=190, n1=40),
            dict(s0=0, n0=100, s1=50, n1=10), dict(s0=50, n0=100, s1=0, n1=51)]
REFUSALS = (
    [("ll_flash_attn", d) for d in (dict(ldq=260), dict(ldo=258), dict(ldk=260), dict(ldq=248), dict(ldo=248), dict(ldk=248), dict(n0=0),
                                    dict(n1=-1), dict(s0=-1), dict(s1=-1), dict(s0=0, n0=100, s1=50, n1=10), dict(s0=50, n0=100, s1=0, n1=51),
                                    dict(s0=0, n0=100, s1=0, n1=100), dict(), dict(B=0, Lq=5), dict(H=0, ldq=0, ldo=0, ldk=0))]
    + [("ll_flash_attn_qnorm", d) for d in (dict(ldq=264), dict(ldo=258), dict(ldk=260), dict(ldo=248), dict(ldk=248), dict(ssq=0),
                                            dict(norm_w=0), dict(key_start=-1), dict(nkeys=0), dict(nkeys=64), dict(nkeys=511),
                                            dict(H=17, ldq=2176, ldo=2176, ldk=2176), dict(), dict(B=0, Lq=5))]
    + [("ll_flash_attn_q", d) for d in (dict(fmt=0), dict(fmt=4), dict(q=0), dict(k=0), dict(v=0), dict(codes=0), dict(scales=0),
                                        dict(B=-1), dict(B=0, Lq=-1), dict(H=0), dict(ldq=260), dict(ldk=260), dict(ldq=248), dict(ldk=248),
                                        dict(ldc=264), dict(ldc=240), dict(fmt=2, ldc=176), dict(fmt=3, ldc=112), dict(lds=6), dict(lds=4),
                                        dict(s0=0, n0=512, s1=256, n1=512), dict(s0=256, n0=512, s1=0, n1=257), dict(n0=64),
                                        dict(s0=0, n0=256, s1=300, n1=256), dict(fmt=2, H=1, ldc=96), dict(n0=0), dict(s0=-1),
                                        dict(), dict(fmt=2, ldc=192), dict(fmt=3, ldc=128), dict(B=0, Lq=5))]
    + [("ll_flash_attn_mx", d) for d in [dict(q=0), dict(out=0), dict(kq=0), dict(ks=0), dict(vq=0), dict(vs=0), dict(head_dim=64),
                                         dict(B=-1), dict(B=0, Lq=-1), dict(H=0), dict(ldq=260), dict(ldo=258), dict(ldq=248), dict(ldo=248)]
       + _SEGS_MX + [dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(), dict(B=0, Lq=5)]]
    + [("ll_flash_attn_mx_q", d) for d in [dict(fmt=0), dict(fmt=4), dict(q=0), dict(codes=0), dict(scales=0), dict(kq=0), dict(ks=0),
                                           dict(vq=0), dict(vs=0), dict(head_dim=64), dict(B=-1), dict(B=0, Lq=-1), dict(H=0),
                                           dict(fmt=2, H=1), dict(fmt=3, H=3), dict(ldq=260), dict(ldq=248), dict(ldc=264), dict(ldc=240),
                                           dict(fmt=2, ldc=176), dict(fmt=3, ldc=112), dict(lds=6), dict(lds=4)]
       + _SEGS_MX + [dict(scale=0.0), dict(scale=float("inf")), dict(), dict(fmt=2, ldc=192), dict(fmt=3, ldc=128), dict(B=0, Lq=5)]])
# (fmt, Lq, H, B, s0, n0, s1, n1, has_out, cap): ll_flash_attn_q_plan's two checks
Q_PLAN_REFUSALS = [(1, 257, 2, 2, 0, 512, 0, 0, 0, 512), (1, 257, 2, 2, 0, 512, 0, 0, 1, 0), (0, 257, 2, 2, 0, 512, 0, 0, 1, 512),
                   (4, 257, 2, 2, 0, 512, 0, 0, 1, 512), (-1, 257, 2, 2, 0, 512, 0, 0, 1, 512)]


def _lib():
    from longlive_amd import _lib as L
    return L.load()


def _tune(lib, t):
    for k in KEYS:
        assert lib.ll_set_tuning(k.encode(), t[k]) == 0


def _err(lib, rc):
    return [rc, lib.ll_last_error().decode() if rc != 0 else ""]


def answers(lib):
    """Every answer the recording holds, as {group: [...]}, under the tunings above; the shipped tuning is restored afterwards."""
    buf = ctypes.create_string_buffer(512)

    def text(rc):
        assert rc == 0
        return buf.value.decode()

    def q_plan(fmt, H, r):      # [return code, the plan, or the error text of a refused fmt]
        rc = lib.ll_flash_attn_q_plan(fmt, 257, H, 2, *r, buf, 512)
        return [rc, buf.value.decode() if rc == 0 else lib.ll_last_error().decode()]

    out = dict(plan=[], q=[], qnorm=[], mx_plan=[], refusals=[], q_plan_refusals=[])
    try:
        for s in PLAN_SETS:
            _tune(lib, s["tuning"])
            out["plan"].append([text(lib.ll_flash_attn_plan(Lq, H, B, n0, n1, adj, buf, 512))
                                for Lq, H, B, n0, n1, adj in itertools.product(*(s[a] for a in AXES))])
        for t in ROUTE_TUNINGS:
            _tune(lib, t)
            out["q"].append([[lib.ll_flash_attn_q_ok(fmt, H, *r)] + q_plan(fmt, H, r) for fmt, H, r in Q_CASES])
            out["qnorm"].append([lib.ll_flash_attn_qnorm_ok(H, n) for H, n in QNORM_CASES])
        _tune(lib, DEFAULTS)
        out["mx_plan"] = [text(lib.ll_flash_attn_mx_plan(Lq, H, B, *r, buf, 512)) for Lq, H, B, r in MX_PLAN_CASES]
        for fn, d in REFUSALS:
            a = dict(BASE[fn], **d)
            assert a["Lq"] <= 0 or a["B"] == 0, (fn, d)      # never a launch, whatever the library makes of the rest
            out["refusals"].append(_err(lib, getattr(lib, fn)(*a.values())))
        for *a, has_out, cap in Q_PLAN_REFUSALS:
            out["q_plan_refusals"].append(_err(lib, lib.ll_flash_attn_q_plan(*a, buf if has_out else None, cap)))
    finally:
        _tune(lib, DEFAULTS)
    return out


def encode(ans):
    """The golden document of answers(): plan strings once, in `strings`, and indices where they are used."""
    index = {}

    def ix(t):
        return index.setdefault(t, len(index))

    doc = dict(plan=[[ix(t) for t in s] for s in ans["plan"]], q=[[[ok, rc, ix(t)] for ok, rc, t in s] for s in ans["q"]],
               qnorm=ans["qnorm"], mx_plan=[ix(t) for t in ans["mx_plan"]], refusals=ans["refusals"],
               q_plan_refusals=ans["q_plan_refusals"])
    doc["strings"] = list(index)
    return doc


def decode(doc):
    s = doc["strings"]
    return dict(plan=[[s[i] for i in p] for p in doc["plan"]], q=[[[ok, rc, s[i]] for ok, rc, i in t] for t in doc["q"]],
                qnorm=doc["qnorm"], mx_plan=[s[i] for i in doc["mx_plan"]], refusals=doc["refusals"],
                q_plan_refusals=doc["q_plan_refusals"])


def _labels():
    """One readable label per answer, in answers()' order per group."""
    lab = dict(plan=[[f"{s['name']} {s['tuning']} {dict(zip(AXES, c))}" for c in itertools.product(*(s[a] for a in AXES))] for s in PLAN_SETS],
               q=[[f"{t} fmt={fmt} H={H} ranges={r}" for fmt, H, r in Q_CASES] for t in ROUTE_TUNINGS],
               qnorm=[[f"{t} H={H} nkeys={n}" for H, n in QNORM_CASES] for t in ROUTE_TUNINGS])
    lab["mx_plan"] = [str(c) for c in MX_PLAN_CASES]
    lab["refusals"] = [f"{fn} {d}" for fn, d in REFUSALS]
    lab["q_plan_refusals"] = [str(c) for c in Q_PLAN_REFUSALS]
    return lab


def _flat(x, nested):
    return list(itertools.chain.from_iterable(x)) if nested else x


def _head(msg):
    """The start of an error text with its formatted numbers taken out: one per LL_REQUIRE."""
    return re.sub(r"-?\d+(\.\d+)?(e[-+]?\d+)?|-?inf|-?nan", "#", msg.split(": ", 1)[1])[:24]


def test_the_recording_covers_every_route_and_every_refusal():
    want = decode(json.load(open(GOLDEN)))
    plans = {re.match(r"\w+(<[^>]*>)?", t).group(0) for s in want["plan"] for t in s}
    assert plans == {"flash_attn_kernel<4>", "flash_attn_pipe_kernel<8, 0>", "flash_attn_pipe_kernel<8, 1>", "flash_attn_asm_kernel"}
    qnames = {t.split(" (")[0] for s in want["q"] for _, _, t in s if t.startswith("flash_attn_asm")}
    assert qnames == {"flash_attn_asm_mx_kernel", "flash_attn_asm_mx6_kernel", "flash_attn_asm_mx4_kernel"}
    assert {ok for s in want["qnorm"] for ok in s} == {0, 1}
    # every refused call is refused in the recording, every other one is an early return with nothing to compute
    for (fn, d), (rc, msg) in zip(REFUSALS, want["refusals"]):
        a = dict(BASE[fn], **d)
        early = d == {} or (a["B"] == 0 and a["Lq"] >= 0) or (fn == "ll_flash_attn" and a["H"] == 0) or d.get("ldc") in (192, 128)
        assert (rc == 0) == early and (rc == 0 or msg.startswith(fn + ":")), (fn, d, rc, msg)
    assert all(rc == -1 and msg.startswith("ll_flash_attn_q_plan:") for rc, msg in want["q_plan_refusals"])
    # one distinct message per LL_REQUIRE (their formatted arguments aside): 4 + 5 + 7 + 10 + 13 + 2
    heads = {fn: {_head(m) for (f, _), (rc, m) in zip(REFUSALS, want["refusals"]) if f == fn and rc} for fn in BASE}
    assert {fn: len(h) for fn, h in heads.items()} == {"ll_flash_attn": 4, "ll_flash_attn_qnorm": 5, "ll_flash_attn_q": 7,
                                                      "ll_flash_attn_mx": 10, "ll_flash_attn_mx_q": 13}, heads
    assert len({_head(m) for _, m in want["q_plan_refusals"]}) == 2


def test_answers_equal_the_recording():
    want = decode(json.load(open(GOLDEN)))
    got = answers(_lib())
    lab = _labels()
    bad = []
    for group in want:
        nested = group in ("plan", "q", "qnorm")
        g, w, names = _flat(got[group], nested), _flat(want[group], nested), _flat(lab[group], nested)
        assert len(g) == len(w) == len(names), group
        bad += [f"{group} {n}: {a!r}, recorded {b!r}" for n, a, b in zip(names, g, w) if a != b]
    assert not bad, f"{len(bad)} answers differ from the recording, the first: " + "; ".join(bad[:5])
