"""One launch per attention route with every stride different from its neighbour's, held to a recording of the bytes the library
wrote before the launches moved into shared launchers (attention.hip: attn_pick + one launch site; attention_asm.hip: fa_launch;
attention_mx.hip: mx_attn_call).  What this file is there for is a swapped stride or pointer in an argument block: B = 2, H = 2,
Lq = 257 (a ragged q-tile and a partial wave), ldq / ldo / ldk padded by 8 / 16 / 24 elements beyond H * 128, the batch stride of the
keys larger than S * ldk, code and scale rows padded by 16 and 4 bytes.  Every output buffer is pre-filled with a byte pattern and
hashed whole (SHA-256), padding included, so a write outside the rows' own bytes shows as well.

tests/golden/attn_route_hashes.json was written by tools/record_attn_goldens.py on an MI355X from that earlier library (recorded
twice, the two recordings equal) and is not to be re-recorded from a later one.

  route                          how it is reached
  flash_attn_kernel<4>           two ranges [3, +64) and [200, +70)
  flash_attn_pipe_kernel<8, 0>   200 keys from slot 5
  flash_attn_pipe_kernel<8, 1>   attn_asm = 0, 1024 keys
  flash_attn_asm_kernel          128 keys, attn_asm_min_keys = 128
  flash_attn_asm_qn_kernel       128 keys (ldq = H * 128: the form's contract)
  flash_attn_asm_mx/mx6/mx4      128 keys
  flash_attn_mx_kernel<0..3>     S = 200, ranges [0, 40) and [70, 200) after kv_shadow_mx over [0, 200) (whose four arrays are hashed
                                 as a route of their own)"""
import ctypes
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_route_hashes.json")
DEFAULTS = dict(attn_variant=2, attn_asm=1, attn_asm_min_keys=512, attn_pp_min_keys=1024, attn_xcd=1)
B, H, LQ, S = 2, 2, 257, 1040
C = H * 128
LDQ, LDO, LDK = C + 8, C + 16, C + 24
KBS = S * LDK + 64
SMX, SMX32 = 200, 224
SCALE = 128 ** -0.5
FILL = 0xA5
BITS = {1: 8, 2: 6, 3: 4}

# name -> (tuning, the kernel its plan must name, the call)
ROUTES = {
    "flash_attn_kernel<4>": (dict(), "flash_attn_kernel<4>", ("bf16", (3, 64, 200, 70))),
    "flash_attn_pipe_kernel<8, 0>": (dict(), "flash_attn_pipe_kernel<8, 0>", ("bf16", (5, 200, 0, 0))),
    "flash_attn_pipe_kernel<8, 1>": (dict(attn_asm=0), "flash_attn_pipe_kernel<8, 1>", ("bf16", (5, 1024, 0, 0))),
    "flash_attn_asm_kernel": (dict(attn_asm_min_keys=128), "flash_attn_asm_kernel", ("bf16", (5, 128, 0, 0))),
    "flash_attn_asm_qn_kernel": (dict(attn_asm_min_keys=128), None, ("qnorm", (5, 128))),
    "flash_attn_asm_mx_kernel": (dict(attn_asm_min_keys=128), "flash_attn_asm_mx_kernel", ("q", 1, (5, 128, 0, 0))),
    "flash_attn_asm_mx6_kernel": (dict(attn_asm_min_keys=128), "flash_attn_asm_mx6_kernel", ("q", 2, (5, 64, 69, 64))),
    "flash_attn_asm_mx4_kernel": (dict(attn_asm_min_keys=128), "flash_attn_asm_mx4_kernel", ("q", 3, (5, 128, 0, 0))),
    "kv_shadow_mx_kernel": (dict(), None, ("shadow",)),
    "flash_attn_mx_kernel<0>": (dict(), None, ("mx", 0)),
    "flash_attn_mx_kernel<1>": (dict(), None, ("mx", 1)),
    "flash_attn_mx_kernel<2>": (dict(), None, ("mx", 2)),
    "flash_attn_mx_kernel<3>": (dict(), None, ("mx", 3)),
}
_state = {}


def _lib():
    from longlive_amd import _lib as L
    return L.load()


def _inputs():
    """The operands of every route, made once from a fixed CPU generator and left unchanged."""
    if _state:
        return _state
    g = torch.Generator(device="cpu").manual_seed(20261019)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)
    bf = torch.bfloat16
    _state.update(
        q=rn(B * LQ, LDQ).to(bf).cuda(), k=rn(B * KBS).to(bf).cuda(), v=rn(B * KBS).to(bf).cuda(),
        qn=(3.0 * rn(B * LQ, C)).to(bf).cuda(), nw=(1.0 + 0.1 * rn(C)).to(bf).cuda(),
        ck=rn(B, SMX, H, 128).to(bf).cuda(), cv=(rn(B, SMX, H, 128) * torch.exp2(torch.arange(H * 128).remainder(7).sub(3).float()).view(H, 128)).to(bf).cuda())
    _state["ssq"] = _state["qn"].float().view(B * LQ, H, 128).square().sum(-1).t().contiguous()      # [H][B * Lq]
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device="cuda")
    sh = [z(B, SMX32, H, 128), z(B, SMX32, H, 4), z(B, H, SMX32 // 32, 128, 32), z(B, H, SMX32 // 32, 128)]
    assert lib.ll_kv_shadow_mx(_state["ck"].data_ptr(), _state["cv"].data_ptr(), *(t.data_ptr() for t in sh), B, SMX, SMX32, H, 128, 0, SMX, st) == 0
    torch.cuda.synchronize()
    _state["shadow"] = sh
    return _state


def _filled(*shape):
    return torch.full(shape, FILL, dtype=torch.uint8, device="cuda")


def run_route(name):
    """{buffer name: SHA-256 of its bytes} of one route's launch; the shipped tuning is restored afterwards."""
    lib, x, st = _lib(), _inputs(), torch.cuda.current_stream().cuda_stream
    tuning, kernel, call = ROUTES[name]
    kind = call[0]
    out = {}
    buf = ctypes.create_string_buffer(512)
    try:
        for k, v in dict(DEFAULTS, **tuning).items():
            assert lib.ll_set_tuning(k.encode(), v) == 0
        if kind == "bf16":
            s0, n0, s1, n1 = call[1]
            assert lib.ll_flash_attn_plan(LQ, H, B, n0, n1, int(n1 > 0 and s1 == s0 + n0), buf, 512) == 0 and buf.value.decode().startswith(kernel)
            out["out"] = _filled(B * LQ, LDO * 2)
            rc = lib.ll_flash_attn(x["q"].data_ptr(), x["k"].data_ptr(), x["v"].data_ptr(), out["out"].data_ptr(), B, LQ, H, LDQ, LDO, LDK, KBS,
                                   s0, n0, s1, n1, SCALE, st)
        elif kind == "qnorm":
            s0, n0 = call[1]
            assert lib.ll_flash_attn_qnorm_ok(H, n0) == 1
            out["out"] = _filled(B * LQ, LDO * 2)
            rc = lib.ll_flash_attn_qnorm(x["qn"].data_ptr(), x["ssq"].data_ptr(), x["nw"].data_ptr(), 1e-6, x["k"].data_ptr(), x["v"].data_ptr(),
                                         out["out"].data_ptr(), B, LQ, H, C, LDO, LDK, KBS, s0, n0, SCALE, st)
        elif kind == "q":
            fmt, r = call[1], call[2]
            assert lib.ll_flash_attn_q_plan(fmt, LQ, H, B, *r, buf, 512) == 0 and buf.value.decode().startswith(kernel + " ")
            ldc, lds = H * 16 * BITS[fmt] + 16, H * 4 + 4
            out["codes"], out["scales"] = _filled(B * LQ, ldc), _filled(B * LQ, lds)
            rc = lib.ll_flash_attn_q(fmt, x["q"].data_ptr(), x["k"].data_ptr(), x["v"].data_ptr(), out["codes"].data_ptr(),
                                     out["scales"].data_ptr(), B, LQ, H, LDQ, ldc, lds, LDK, KBS, *r, SCALE, st)
        elif kind == "shadow":
            out.update(zip(("kq", "ks", "vq", "vs"), x["shadow"]))
            rc = 0
        else:
            fmt = call[1]
            sh = [t.data_ptr() for t in x["shadow"]]
            if fmt == 0:
                out["out"] = _filled(B * LQ, LDO * 2)
                rc = lib.ll_flash_attn_mx(x["q"].data_ptr(), *sh, out["out"].data_ptr(), B, LQ, H, 128, LDQ, LDO, SMX, SMX32, 0, 40, 70, 130,
                                          SCALE, st)
            else:
                ldc, lds = H * 16 * BITS[fmt] + 16, H * 4 + 4
                out["codes"], out["scales"] = _filled(B * LQ, ldc), _filled(B * LQ, lds)
                rc = lib.ll_flash_attn_mx_q(fmt, x["q"].data_ptr(), *sh, out["codes"].data_ptr(), out["scales"].data_ptr(), B, LQ, H, 128, LDQ,
                                            ldc, lds, SMX, SMX32, 0, 40, 70, 130, SCALE, st)
        assert rc == 0, lib.ll_last_error().decode()
        torch.cuda.synchronize()
        assert all(bool((t != FILL).any()) for t in out.values()), "a buffer nothing was written to"
    finally:
        for k, v in DEFAULTS.items():
            lib.ll_set_tuning(k.encode(), v)
    return {n: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for n, t in out.items()}


@pytest.mark.parametrize("name", list(ROUTES))
def test_route_writes_the_recorded_bytes(name):
    want = json.load(open(GOLDEN))
    assert set(want) == set(ROUTES)
    got = run_route(name)
    assert got == want[name], f"{name}: " + ", ".join(n for n in got if got[n] != want[name].get(n))
