"""Host-side checks of the attention entry points with quantised output (include/longlive_hip.h: ll_flash_attn_q_ok, ll_flash_attn_q,
ll_flash_attn_q_plan, ll_flash_attn_mx_q): the binding and the library agree on them at ABI 111, the eligibility rule, the refusal
where it says no, and the model's mode table naming the format the mode's GEMMs read."""
import ctypes as C

import pytest

from longlive_amd import _lib

MX, MX6, MX4 = 1, 2, 3
NEW = ("ll_flash_attn_q_ok", "ll_flash_attn_q", "ll_flash_attn_q_plan", "ll_flash_attn_mx_q")


def test_binding_and_library_hold_the_new_entry_points_at_abi_111():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.ll_version() == 111 == _lib.ABI_VERSION


@pytest.mark.parametrize("fmt,H,segs,want", [
    (MX, 2, (0, 64, 128, 512), 0),          # two ranges with a gap
    (MX, 2, (0, 192, 192, 600), 1),         # adjacent: one range of 792
    (MX4, 12, (0, 192, 192, 600), 1),
    (MX, 2, (3, 512, 0, 0), 1),             # the default minimum of the generated kernel
    (MX, 2, (3, 511, 0, 0), 0),             # one key short of it
    (MX6, 2, (0, 100, 0, 0), 0),            # fewer than two key tiles
    (MX6, 3, (0, 512, 0, 0), 0),            # packed formats pair heads
    (MX4, 3, (0, 512, 0, 0), 0),
    (MX, 3, (0, 512, 0, 0), 1),
    (0, 2, (0, 512, 0, 0), 0),              # not a format
    (4, 2, (0, 512, 0, 0), 0),
])
def test_q_ok_truth_table(fmt, H, segs, want):
    assert _lib.load().ll_flash_attn_q_ok(fmt, H, *segs) == want


def test_q_ok_follows_the_tuning_key():
    lib = _lib.load()
    assert lib.ll_flash_attn_q_ok(MX, 2, 0, 128, 0, 0) == 0
    try:
        assert lib.ll_set_tuning(b"attn_asm_min_keys", 128) == 0
        assert lib.ll_flash_attn_q_ok(MX, 2, 0, 128, 0, 0) == 1
        assert lib.ll_flash_attn_q_ok(MX, 2, 0, 127, 0, 0) == 0       # two key tiles whatever the key says
        assert lib.ll_set_tuning(b"attn_asm", 0) == 0
        assert lib.ll_flash_attn_q_ok(MX, 2, 0, 512, 0, 0) == 0
    finally:
        lib.ll_set_tuning(b"attn_asm", 1)
        lib.ll_set_tuning(b"attn_asm_min_keys", 512)


@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_flash_attn_q(MX, 1, 1, 1, 1, 1, 1, 128, 2, 256, 256, 8, 256, 0, 0, 64, 128, 512, 0.088, None), "not covered"),
    (lambda L: L.ll_flash_attn_q(MX6, 1, 1, 1, 1, 1, 1, 128, 3, 384, 288, 12, 384, 0, 0, 512, 0, 0, 0.088, None), "not covered"),
    (lambda L: L.ll_flash_attn_q(7, 1, 1, 1, 1, 1, 1, 128, 2, 256, 256, 8, 256, 0, 0, 512, 0, 0, 0.088, None), "fmt=7"),
    (lambda L: L.ll_flash_attn_q(MX4, 1, 1, 1, 1, 1, 1, 128, 2, 256, 64, 8, 256, 0, 0, 512, 0, 0, 0.088, None), "code row stride"),
    (lambda L: L.ll_flash_attn_q(MX, 1, 1, 1, 1, None, 1, 128, 2, 256, 256, 8, 256, 0, 0, 512, 0, 0, 0.088, None), "required"),
    (lambda L: L.ll_flash_attn_mx_q(MX6, 1, 1, 1, 1, 1, 1, 1, 1, 128, 3, 128, 384, 288, 12, 64, 64, 0, 64, 0, 0, 0.088, None), "even"),
    (lambda L: L.ll_flash_attn_mx_q(MX, 1, 1, 1, 1, 1, 1, 1, 1, 128, 2, 128, 256, 256, 8, 70, 64, 0, 64, 0, 0, 0.088, None), "S32"),
])
def test_refusals_before_any_launch(call, needle):
    lib = _lib.load()
    assert call(lib) == -1
    assert needle in lib.ll_last_error().decode(), lib.ll_last_error().decode()


def test_plan_names_the_kernel_or_the_two_launches():
    lib = _lib.load()
    buf = C.create_string_buffer(512)
    assert lib.ll_flash_attn_q_plan(MX4, 4680, 12, 1, 0, 512, 0, 0, buf, 512) == 0
    assert "flash_attn_asm_mx4_kernel" in buf.value.decode() and "228 workgroups" in buf.value.decode(), buf.value
    assert lib.ll_flash_attn_q_plan(MX6, 4680, 12, 1, 0, 64, 128, 512, buf, 512) == 0
    assert "ll_flash_attn + ll_quantize_mx6" in buf.value.decode(), buf.value


def test_mode_table_names_the_activation_format_of_the_modes_gemms():
    from longlive_amd import model, ops
    gemms = {"mxfp8": ops.gemm_mx, "mxfp6": ops.gemm_mx6, "mxfp4_a6": ops.gemm_mx4w6, "mxfp4_a4": ops.gemm_mx4}
    for mode, gemm in gemms.items():
        afmt = gemm.args[1]                      # _bind(_qgemm, entry, afmt, wfmt)
        assert model._QUANT_MODES[mode].afmt is afmt and afmt in (ops.MX, ops.MX6, ops.MX4), mode
    for mode in (None, "int8", "fp8_rowwise"):
        assert model._QUANT_MODES[mode].afmt is None, mode
    assert set(model._QUANT_MODES) == set(gemms) | {None, "int8", "fp8_rowwise"}
